// percall.cpp — the host-buffer ("per-call") tier of include/chunky_ec.h: the
// calls that take the caller's host memory, one part or a few buffers at a time, stage it on the
// device and run the launch steps of capi.cpp over it.  Staging contexts, the per-part
// encode / reconstruct, and the coalescer that makes concurrent calls share a launch.
#include "capi_internal.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>

#include "hostmem.hpp"

using namespace cec;

namespace {

// ------------------------------------------------------------------------------------------
// Staging contexts for the host-buffer API: a stream + a device buffer, leased per call from a
// bounded per-device pool (not thread_local: the reference calls the crate from tokio's
// blocking pool, whose threads come and go, file_part.rs:128,161 / any.rs:19-24, so per-thread
// resources would leak with every retired thread).  At most kMaxIdleCtx contexts per device
// stay alive between calls, holding at most CEC_IDLE_STAGING_MIB (default 1 GiB) of device
// buffers together; cec_release_cached() frees the idle ones.
// ------------------------------------------------------------------------------------------
// Device bytes idle contexts may hold per device (knobs().idle_staging_bytes, the
// CEC_IDLE_STAGING_MIB knob, default 1 GiB).  Bounding the total (not each buffer) keeps a
// steady stream of large per-call requests (e.g. RS(10,4) at 8 MiB chunks: 112 MiB per part)
// from paying a hipMalloc + a device-synchronizing hipFree on every call.

class CtxPool {
   public:
    using Ctx = StageCtx;
    // Leaked on purpose: destroying HIP objects from a static destructor races the runtime's own
    // teardown at process exit.
    static CtxPool& get() {
        static CtxPool* pool = new CtxPool();
        return *pool;
    }
    // An idle context of `device` whose buffer already holds `device_bytes` (the smallest such),
    // else the one with the largest buffer (grown by ctx_reserve), else a new one.
    std::unique_ptr<StageCtx> take(int device, size_t device_bytes) {
        std::lock_guard<std::mutex> lk(mu_);
        auto& v = idle_[device];
        if (v.empty()) {
            auto c = std::make_unique<StageCtx>();
            c->device = device;
            return c;
        }
        size_t best = 0;
        for (size_t i = 1; i < v.size(); ++i) {
            const size_t a = v[i]->dcap, b = v[best]->dcap;
            const bool fits_a = a >= device_bytes, fits_b = b >= device_bytes;
            if (fits_a != fits_b ? fits_a : (fits_a ? a < b : a > b)) best = i;
        }
        auto c = std::move(v[best]);
        v.erase(v.begin() + std::ptrdiff_t(best));
        idle_bytes_[device] -= c->dcap;
        return c;
    }
    static int prepare(StageCtx& c, size_t device_bytes) { return ctx_reserve(c, device_bytes); }
    // The caller's current device is the context's (leases never cross devices).
    void give(std::unique_ptr<StageCtx> c) {
        if (!c) return;
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        bool drop_buffer = false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto& v = idle_[c->device];
            if (v.size() < kMaxIdleCtx) {
                size_t& held = idle_bytes_[c->device];
                if (held + c->dcap <= knobs().idle_staging_bytes) {
                    held += c->dcap;
                    v.push_back(std::move(c));
                    return;
                }
                drop_buffer = true;  // over the budget: keep the stream, free the buffer below
            }
        }
        if (!drop_buffer) {
            c->destroy();
            return;
        }
        c->release_buffer();
        std::lock_guard<std::mutex> lk(mu_);
        auto& v = idle_[c->device];
        if (v.size() < kMaxIdleCtx) v.push_back(std::move(c));
        // (else another thread filled the pool meanwhile: c's stream is destroyed with it)
    }

    // Destroys the idle contexts of `device` (every device if < 0): their streams and device
    // buffers are freed; leased contexts are untouched.  Returns the device bytes released.
    size_t trim(int device) {
        std::vector<std::unique_ptr<StageCtx>> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (auto& [dev, v] : idle_) {
                if (device >= 0 && dev != device) continue;
                for (auto& c : v) out.push_back(std::move(c));
                v.clear();
                idle_bytes_[dev] = 0;
            }
        }
        size_t bytes = 0;
        int cur = 0;
        const bool have_cur = hipGetDevice(&cur) == hipSuccess;
        for (auto& c : out) {
            bytes += c->dcap;
            if (hipSetDevice(c->device) == hipSuccess) c->destroy();
            (void)hipGetLastError();
        }
        if (have_cur) (void)hipSetDevice(cur);
        return bytes;
    }

   private:
    std::mutex mu_;
    std::map<int, std::vector<std::unique_ptr<StageCtx>>> idle_;
    std::map<int, size_t> idle_bytes_;
};

// Crate checks shared by the per-part reconstruct entry points.  Returns CEC_OK with *len set
// and *work = true if something must be rebuilt.
int check_reconstruct(const cec_codec* c, const size_t* lens, const uint8_t* present,
                      size_t n_shards, size_t* len, bool* work) {
    const size_t t = c->d + c->p;
    if (n_shards < t) return CEC_TOO_FEW_SHARDS;
    if (n_shards > t) return CEC_TOO_MANY_SHARDS;
    size_t n_present = 0;
    bool have = false;
    for (size_t i = 0; i < t; ++i) {
        if (!present[i]) continue;
        if (lens[i] == 0) return CEC_EMPTY_SHARD;
        ++n_present;
        if (have && lens[i] != *len) return CEC_INCORRECT_SHARD_SIZE;
        *len = lens[i];
        have = true;
    }
    *work = n_present != t;
    if (!*work) return CEC_OK;
    if (n_present < c->d) return CEC_TOO_FEW_SHARDS_PRESENT;
    return CEC_OK;
}

int reconstruct_host(const cec_codec* cc, uint8_t* const* shards, const size_t* lens,
                     uint8_t* present, size_t n_shards, bool data_only) {
    if (!cc || !shards || !lens || !present) return CEC_ERR_INVALID_ARGUMENT;
    cec_codec* c = const_cast<cec_codec*>(cc);
    size_t len = 0;
    bool work = false;
    CEC_TRY(check_reconstruct(c, lens, present, n_shards, &len, &work));
    if (!work) return CEC_OK;
    const size_t t = c->d + c->p;
    auto rec = c->decode_record(make_key(present, t, data_only));
    const size_t n_out = (*rec)[0];
    const uint32_t* out_idx = rec->data() + 1 + c->d;
    for (size_t k = 0; k < n_out; ++k) {
        const size_t o = out_idx[k];
        if (!shards[o] || lens[o] < len) {
            set_last_error("missing shard buffer too small");
            return CEC_ERR_INVALID_ARGUMENT;
        }
    }
    if (n_out == 0) return CEC_OK;  // data_only with only parity missing
    const size_t cs = round_up(len, kChunkAlign);
    const size_t rec_bytes = round_up(rec->size() * sizeof(uint32_t), kChunkAlign);
    Lease<CtxPool> ctx;
    CEC_TRY(ctx.acquire(rec_bytes + t * cs));
    uint32_t* drec = reinterpret_cast<uint32_t*>(ctx->dbuf);
    uint8_t* dbase = ctx->dbuf + rec_bytes;
    HIP_TRY(hipMemcpyAsync(drec, rec->data(), rec->size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* in_idx = rec->data() + 1;
    for (size_t j = 0; j < c->d; ++j)
        HIP_TRY(hipMemcpyAsync(dbase + in_idx[j] * cs, shards[in_idx[j]], len,
                               hipMemcpyHostToDevice, ctx->stream));
    const cec_part_batch b{dbase, t * cs, cs, 1, len};
    HIP_TRY(launch_decode(b, c->d, drec, nullptr, uint32_t(n_out), 0, ctx->stream));
    for (size_t k = 0; k < n_out; ++k)
        HIP_TRY(hipMemcpyAsync(shards[out_idx[k]], dbase + out_idx[k] * cs, len,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < n_out; ++k) present[out_idx[k]] = 1;
    return CEC_OK;
}

// ------------------------------------------------------------------------------------------
// Per-call coalescing ("a batch queue behind the per-part call").
//
// A GPU SHA-256 lane hashes one chunk as a serial chain (~42 ms per MiB), so one part per
// launch leaves the chip idle and the reference's own concurrency (≤10 part tasks,
// writer.rs:130; `concurrency` is a builder knob) only helps if concurrent calls share a
// launch.  cec_part_encode / cec_sha256(_many) therefore go through a leader/follower queue:
// the first caller to find no batch in progress becomes the leader, waits up to
// CEC_COALESCE_US microseconds (default 200; only when calls are concurrent) for more requests
// with its key (the device; for cec_part_encode the codec too, and the chunk length while
// CEC_COALESCE_MIXED is 0; for cec_part_read the codec and the mode), and runs them as ONE batch:
//   1. copy-in   every caller copies its own (pageable) input into the queue's pinned staging,
//                in parallel on its own thread;
//   2. launch    the leader moves the whole batch with one H2D copy, runs the fused
//                encode+hash (or the SHA) kernel over every part, and brings parity and
//                digests back with one D2H copy into pinned staging;
//   3. copy-out  every caller copies its results out into its own buffers, in parallel.
// Batches are capped at CEC_COALESCE_MAX_MIB of input (default 1024).  Results are
// bit-identical to one call per launch (same kernels, same inputs).
// cec_part_encode calls of different chunk lengths share a batch in the split layout of the ragged
// encode (PartImpl below); cec_part_read, the read side's per-part call, has a queue of its own
// whose batches are rounds of cec_parts_read (ReadImpl).
// ------------------------------------------------------------------------------------------
// cec_coalesce_stats (cec_sha256(_many) and cec_part_encode) and cec_coalesce_detail (batches of
// cec_part_encode calls of two or more chunk lengths; cec_part_read calls and their launches).
struct Counters {
    std::atomic<uint64_t> calls{0}, launches{0};
};
Counters g_write_counters, g_read_counters;
std::atomic<uint64_t> g_mixed_batches{0};

// What an unset CEC_COALESCE_MIXED selects.  The rule, fixed before the measurement: gathering
// across chunk lengths becomes the default only if (1) on the small-file workload its worst repeat
// beats the by-length arm's best at every shape and thread count, and (2) with uniform callers
// (RS(10,4), 1 MiB chunks, 10 / 64 / 256 callers, where both values run the same batch code) no
// arm's worst repeat lies outside the other's range by more than that arm's own spread.  (1) holds
// everywhere, by 2.5-2.9 times at 10 threads and 20-27 times at 256
// (profiles/small_files/percall_mixed.log).  (2) does not: 64 pageable callers gave 12.54-13.30
// GB/s at 0 and 12.18-12.33 at 1 (profiles/small_files/percall_uniform.log), 0.36 below the
// other's range with a spread of 0.15.  So unset = 0 and the path is reached through the knob.
constexpr bool kCoalesceMixedDefault = false;
inline bool gather_mixed() {
    const int m = knobs().coalesce_mixed;
    return m >= 0 ? m == 1 : kCoalesceMixedDefault;
}

// What the calls of one batch share.  `what`: the chunk length while cec_part_encode gathers by
// length (CEC_COALESCE_MIXED=0), cec_part_read's mode, else 0.
struct CoalesceKey {
    const void* codec;
    size_t what;
    int device;
    bool operator==(const CoalesceKey& o) const {
        return codec == o.codec && what == o.what && device == o.device;
    }
};

enum class Phase { Queued, CopyIn, Staged, CopyOut, Finished };

struct ReqBase {
    int device = 0;
    int status = CEC_OK;
    std::string err;
    Phase phase = Phase::Queued;
    size_t slot = 0;        // index in the batch
    size_t in_off = 0;      // byte offset in the pinned input staging
    size_t item0 = 0;       // sha: first item index; parts: offset of the digest block
    Arena* arena = nullptr;
    struct Batch* batch = nullptr;  // the batch this request runs in
    std::condition_variable cv;     // this caller's wake-ups
};

// Impl: cap_bytes(r) = weight against the cap; prepare(batch, arena) lays out + reserves;
// copy_in(r); run(batch, arena) launches and waits; copy_out(r); counters(), what its calls and
// launches count into; arenas(), the pool its batches take their arena from (at most
// knobs().coalesce_inflight in use per queue).
// Wake-ups are targeted (one condition variable per request plus one for the leader) so a
// batch of hundreds of callers costs O(batch) wake-ups, not O(batch^2).
// One batch in flight: its size and copy counters, and the leader's wake-ups.
struct Batch {
    size_t size = 0, staged = 0, finished = 0;
    std::condition_variable cv;
};

template <typename Req, typename Impl>
class Coalescer {
   public:
    int submit(Req* r) {
        Impl::counters().calls.fetch_add(1, std::memory_order_relaxed);
        std::unique_lock<std::mutex> lk(mu_);
        peak_ = std::max(peak_, ++callers_);
        queue_.push_back(r);
        if (gathering_) gather_cv_.notify_one();  // the gathering leader re-checks its batch
        for (;;) {
            if (r->phase == Phase::CopyIn) {
                lk.unlock();
                Impl::copy_in(*r);
                lk.lock();
                r->phase = Phase::Staged;
                if (++r->batch->staged == r->batch->size) r->batch->cv.notify_one();
            } else if (r->phase == Phase::CopyOut) {
                lk.unlock();
                if (r->status == CEC_OK) Impl::copy_out(*r);
                lk.lock();
                r->phase = Phase::Finished;
                if (++r->batch->finished == r->batch->size) r->batch->cv.notify_one();
                break;
            } else if (r->phase == Phase::Queued && r->batch == nullptr && !gathering_ &&
                       (active_ == 0 || (overflow_ && active_ < knobs().coalesce_inflight))) {
                // Batches on the GPU at once (CEC_COALESCE_INFLIGHT, 1..16; default 2).  A second
                // batch starts while one runs only when the batch before it overflowed the cap
                // (callers of its key were left queued): otherwise a leader would start as soon
                // as an arena is free, and since a launch costs one chunk's SHA chain whatever
                // its size, the callers would split into ever smaller batches that each pay it
                // (round 1, unconditional: 100 threads 7.1-8.2 GB/s with 1 vs 3.6-3.8 with 4,
                // profiles/r1y_percall_ab.log).  Overflowing callers (256 pageable parts vs a
                // 1 GiB cap) then copy in while the first batch runs: 13.9 -> ~26 GB/s
                // (profiles/r2_percall/).
                // r->batch: a caller already taken into a batch stays Queued until its leader
                // has prepared the arena (lock released meanwhile); woken in that window (a
                // wake-up sent before the batch formed) it must not lead a batch of its own, or
                // it never copies in and its leader waits forever — seen with two batches in
                // flight at 256 pageable callers.
                lead(r, lk);
                break;
            } else {
                r->cv.wait(lk);
            }
        }
        --callers_;
        lk.unlock();
        if (r->status != CEC_OK) set_last_error(r->err);
        return r->status;
    }

   private:
    // Wake the oldest queued request so it can lead the next batch (if a slot is free).
    void wake_next() {
        if (!queue_.empty()) queue_.front()->cv.notify_one();
    }

    // Called with lk held; returns with r finished.  Up to knobs().coalesce_inflight leaders run
    // their batches at once (one arena = pinned staging + device buffer + stream each), so the
    // next batch gathers, copies and launches while earlier ones are still on the GPU.
    void lead(Req* r, std::unique_lock<std::mutex>& lk) {
        ++active_;
        gathering_ = true;
        const bool trace = knobs().coalesce_trace;
        const auto key = r->key();
        auto matching_bytes = [&] {
            size_t b = 0;
            for (Req* q : queue_)
                if (q->key() == key) b += Impl::cap_bytes(*q);
            return b;
        };
        auto matching_count = [&] {
            size_t n = 0;
            for (Req* q : queue_) n += q->key() == key ? 1 : 0;
            return n;
        };
        if (last_batch_ > 1 || queue_.size() > 1) {
            // Wait for company only when calls are actually concurrent (the last batch had several
            // callers, or others are queued now): a lone caller's calls never pay the window.
            // The window scales with the last launch (1/8 of its run time, at least
            // CEC_COALESCE_US): callers of the batch that just finished are still copying their
            // results out and come back a few ms later; a short window splits the callers into
            // two alternating groups, each paying a full launch (10 threads: 5 parts per launch).
            // It ends early once as many callers are queued as were ever inside at once lately.
            const uint64_t window = std::max<uint64_t>(knobs().coalesce_us, last_run_us_ / 8);
            const auto until =
                std::chrono::steady_clock::now() + std::chrono::microseconds(window);
            gather_cv_.wait_until(lk, until, [&] {
                return matching_bytes() >= coalesce_max_bytes() || matching_count() >= peak_;
            });
        }
        Batch batch_state;
        std::vector<Req*> batch{r};
        size_t bytes = Impl::cap_bytes(*r);
        for (auto it = queue_.begin(); it != queue_.end();) {
            if (*it == r) {
                it = queue_.erase(it);
            } else if ((*it)->key() == key &&
                       bytes + Impl::cap_bytes(**it) <= coalesce_max_bytes()) {
                bytes += Impl::cap_bytes(**it);
                batch.push_back(*it);
                it = queue_.erase(it);
            } else {
                ++it;
            }
        }
        for (Req* q : batch) q->batch = &batch_state;
        batch_state.size = batch.size();
        last_batch_ = batch.size();
        overflow_ = false;  // callers of this key left behind by the cap
        for (Req* q : queue_) overflow_ = overflow_ || q->key() == key;
        if (++batches_since_peak_ >= 32) {  // forget an old burst of callers
            peak_ = callers_;
            batches_since_peak_ = 0;
        }
        Arena* arena = Impl::arenas().take(key.device);
        gathering_ = false;
        if (trace)
            std::fprintf(stderr, "[cec coalesce] lead arena %p: %zu callers, %u active, %zu queued\n",
                         (void*)arena, batch.size(), active_, queue_.size());
        wake_next();  // the next batch can gather while this one runs
        lk.unlock();
        const auto t0 = std::chrono::steady_clock::now();
        auto t1 = t0, t2 = t0, t3 = t0;
        int st = Impl::prepare(batch, *arena);
        if (trace)
            std::fprintf(stderr, "[cec coalesce] arena %p: prepared (%d)\n", (void*)arena, st);
        if (st == CEC_OK) {
            lk.lock();
            batch_state.staged = 1;  // the leader's own copy, done below
            for (Req* q : batch)
                if (q != r) {
                    q->phase = Phase::CopyIn;
                    q->cv.notify_one();
                }
            t1 = std::chrono::steady_clock::now();
            lk.unlock();
            Impl::copy_in(*r);
            lk.lock();
            batch_state.cv.wait(lk, [&] { return batch_state.staged == batch_state.size; });
            lk.unlock();
            if (trace) std::fprintf(stderr, "[cec coalesce] arena %p: staged\n", (void*)arena);
            t2 = std::chrono::steady_clock::now();
            Impl::counters().launches.fetch_add(1, std::memory_order_relaxed);
            st = Impl::run(batch, *arena);
            t3 = std::chrono::steady_clock::now();
        }
        const std::string err = st == CEC_OK ? std::string() : last_error();
        lk.lock();
        last_run_us_ = uint64_t(std::chrono::duration_cast<std::chrono::microseconds>(t3 - t2).count());
        batch_state.finished = 1;
        for (Req* q : batch) {
            q->status = st;
            q->err = err;
            if (q != r) {
                q->phase = Phase::CopyOut;
                q->cv.notify_one();
            }
        }
        lk.unlock();
        if (st == CEC_OK) Impl::copy_out(*r);
        lk.lock();
        // the arena is reused by a later batch: wait for every copy-out
        batch_state.cv.wait(lk, [&] { return batch_state.finished == batch_state.size; });
        if (trace) {
            auto ms = [](auto a, auto b) {
                return std::chrono::duration<double, std::milli>(b - a).count();
            };
            std::fprintf(stderr,
                         "[cec coalesce] batch %zu (%zu B): prepare %.2f ms, copy-in %.2f ms, "
                         "run %.2f ms, copy-out %.2f ms\n",
                         batch.size(), bytes, ms(t0, t1), ms(t1, t2), ms(t2, t3),
                         ms(t3, std::chrono::steady_clock::now()));
        }
        r->phase = Phase::Finished;
        Impl::arenas().give(key.device, arena);
        --active_;
        wake_next();
    }

    std::mutex mu_;
    std::condition_variable gather_cv_;
    std::deque<Req*> queue_;
    bool gathering_ = false;
    uint32_t active_ = 0;
    bool overflow_ = false;          // the last batch formed left callers of its key queued
    size_t last_batch_ = 0;
    size_t callers_ = 0;             // submit() calls in progress
    size_t peak_ = 0;                // most callers in progress at once, lately
    uint32_t batches_since_peak_ = 0;
    uint64_t last_run_us_ = 0;       // launch-to-results time of the last batch
};

// ---- cec_sha256(_many): one request = n buffers ----
struct ShaReq : ReqBase {
    const uint8_t* const* bufs = nullptr;
    const size_t* lens = nullptr;
    size_t n = 0;
    uint8_t* out = nullptr;
    CoalesceKey key() const { return {nullptr, 0, device}; }
};

// The arenas of the cec_sha256(_many) and the cec_part_encode queue: kept for the process.
template <typename Tag>
ArenaPool& own_arenas() {
    static ArenaPool* pool = new ArenaPool();
    return *pool;
}

struct ShaImpl {
    static Counters& counters() { return g_write_counters; }
    static ArenaPool& arenas() { return own_arenas<ShaImpl>(); }
    static size_t item_bytes(size_t len) { return round_up(std::max<size_t>(len, 1), kChunkAlign); }
    static size_t bytes(const ShaReq& r) {
        size_t b = 0;
        for (size_t i = 0; i < r.n; ++i) b += item_bytes(r.lens[i]);
        return b;
    }
    static size_t cap_bytes(const ShaReq& r) { return bytes(r); }
    static int prepare(std::vector<ShaReq*>& batch, Arena& a) {
        size_t off = 0, items = 0;
        for (ShaReq* r : batch) {
            r->arena = &a;
            r->in_off = off;
            r->item0 = items;
            off += bytes(*r);
            items += r->n;
        }
        CEC_TRY(a.in.reserve(off, coalesce_max_bytes()));
        CEC_TRY(a.out.reserve(items * 32, coalesce_max_bytes() / 8));
        const size_t meta = round_up(2 * items * sizeof(uint64_t), kChunkAlign);
        return ctx_reserve(a.dev, meta + round_up(items * 32, kChunkAlign) + off);
    }
    static void copy_in(ShaReq& r) {
        size_t off = r.in_off;
        for (size_t i = 0; i < r.n; ++i) {
            if (r.lens[i]) std::memcpy(r.arena->in.ptr + off, r.bufs[i], r.lens[i]);
            off += item_bytes(r.lens[i]);
        }
    }
    static int run(std::vector<ShaReq*>& batch, Arena& a) {
        size_t items = 0, total = 0;
        for (ShaReq* r : batch) {
            items += r->n;
            total += bytes(*r);
        }
        const size_t meta = round_up(2 * items * sizeof(uint64_t), kChunkAlign);
        const size_t dig = round_up(items * 32, kChunkAlign);
        uint64_t* dptrs = reinterpret_cast<uint64_t*>(a.dev.dbuf);
        uint8_t* ddig = a.dev.dbuf + meta;
        uint8_t* ddata = ddig + dig;
        std::vector<uint64_t> hmeta(2 * items);
        size_t k = 0, off = 0;
        for (ShaReq* r : batch)
            for (size_t i = 0; i < r->n; ++i, ++k) {
                hmeta[k] = reinterpret_cast<uint64_t>(ddata + off);
                hmeta[items + k] = r->lens[i];
                off += item_bytes(r->lens[i]);
            }
        hipStream_t s = a.dev.stream;
        HIP_TRY(hipMemcpyAsync(ddata, a.in.ptr, total, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dptrs, hmeta.data(), hmeta.size() * sizeof(uint64_t),
                               hipMemcpyHostToDevice, s));
        // list mode: not a cec_part_batch layout
        const ShaParams h = sha_list_params(dptrs, dptrs + items, items, nullptr, 0, ddig);
        HIP_TRY(launch_sha256(h, true, s));
        HIP_TRY(hipMemcpyAsync(a.out.ptr, ddig, items * 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return CEC_OK;
    }
    static void copy_out(ShaReq& r) {
        std::memcpy(r.out, r.arena->out.ptr + r.item0 * 32, r.n * 32);
    }
};

// ---- cec_part_encode: one request = one part (d*L bytes of data_buf) ----
struct PartReq : ReqBase {
    cec_codec* codec = nullptr;
    const uint8_t* data_buf = nullptr;  // d*L bytes
    size_t L = 0;
    uint8_t* parity_out = nullptr;      // p*L bytes
    uint8_t* digests_out = nullptr;     // (d+p)*32 bytes
    // Page-locked caller buffers (cec_host_alloc): DMA'd directly, no copy-in / copy-out.
    bool in_pinned = false, out_pinned = false;
    plan::PartPlace at{};               // this part's places in the batch (percall_plan.hpp)
    uint8_t* dbuf = nullptr;            // the batch's device buffer
    hipStream_t stream = nullptr;       // the batch's stream
    // Any lengths together, or (CEC_COALESCE_MIXED=0) one chunk length per batch.
    CoalesceKey key() const { return {codec, gather_mixed() ? 0 : L, device}; }
};

// The layout is plan::part_layout's (percall_plan.hpp).  A batch of one chunk length: pinned input
// [part][d][cs] (staged parts only, at in_off), output [part][p][cs] (staged parts only, at
// out_off) then digests [part][d+p][32]; device batch [part][d+p][cs] (cs = L rounded up to
// 256 B), encoded by encode_hash_steps with the parity brought back early on a side stream.  A
// batch of two or more lengths: the split layout, rows at L rounded up to 16, a data and a parity
// region behind the digest block, encoded and hashed by ragged_launch (which has no hook for an
// early parity download: it comes back behind the SHA-256 launch).  Either way a batch with no
// page-locked caller buffer moves with one copy each way; otherwise every part is copied on its
// own (pinned ones straight from / into the caller's memory).
struct PartImpl {
    static Counters& counters() { return g_write_counters; }
    static ArenaPool& arenas() { return own_arenas<PartImpl>(); }
    static size_t bytes(const PartReq& r) { return r.codec->d * round_up(r.L, kChunkAlign); }
    // Weight against CEC_COALESCE_MAX_MIB: the cap bounds the pinned staging a batch needs; a
    // page-locked caller needs none, so its part counts a quarter (its batch is bounded by the
    // device buffer, 4x the staging cap).
    // (A/B at 256 page-locked callers, profiles/r2_percall/pinned_cap_*: full weight 26.0 GB/s,
    // half 23.6, quarter 24.8 — noise; the quarter keeps them in one launch.)
    static size_t cap_bytes(const PartReq& r) { return r.in_pinned ? bytes(r) / 4 : bytes(r); }
    static bool any_pinned(const std::vector<PartReq*>& batch) {
        for (const PartReq* r : batch)
            if (r->in_pinned || r->out_pinned) return true;
        return false;
    }
    static plan::PartTotals layout(const std::vector<PartReq*>& batch,
                                   std::vector<plan::PartPlace>* at) {
        const cec_codec* c = batch[0]->codec;
        std::vector<plan::PartIn> in;
        for (const PartReq* r : batch) in.push_back({r->L, r->in_pinned, r->out_pinned});
        at->resize(batch.size());
        plan::PartTotals tot{};
        plan::part_layout(c->d, c->p, in.data(), in.size(), at->data(), &tot);
        return tot;
    }
    static int prepare(std::vector<PartReq*>& batch, Arena& a) {
        const cec_codec* c = batch[0]->codec;
        const size_t d = c->d, p = c->p, t = d + p;
        std::vector<plan::PartPlace> at;
        const plan::PartTotals tot = layout(batch, &at);
        const size_t cap = coalesce_max_bytes();
        CEC_TRY(a.in.reserve(std::max<size_t>(tot.in_bytes, 1), cap));
        CEC_TRY(a.out.reserve(tot.out_bytes + tot.dig_bytes,
                              cap / d * p + (tot.mixed ? cap / 8 : cap / at[0].stride * t * 32)));
        CEC_TRY(ctx_reserve(a.dev, tot.dev_bytes));
        for (size_t k = 0; k < batch.size(); ++k) {
            PartReq* r = batch[k];
            r->arena = &a;
            r->slot = k;
            r->at = at[k];
            r->in_off = at[k].in_off;
            r->item0 = tot.out_bytes;  // locates the digest block
            r->dbuf = a.dev.dbuf;
            r->stream = a.dev.stream;
        }
        return CEC_OK;
    }
    // This part's upload into the device batch (from the caller's page-locked buffer or from its
    // copy in the pinned staging).
    static hipError_t upload(PartReq& r) {
        const size_t d = r.codec->d, cs = r.at.stride;
        uint8_t* dst = r.dbuf + r.at.dev_data;
        if (r.in_pinned && cs == r.L)
            return hipMemcpyAsync(dst, r.data_buf, d * r.L, hipMemcpyHostToDevice, r.stream);
        if (r.in_pinned)
            return hipMemcpy2DAsync(dst, cs, r.data_buf, r.L, r.L, d, hipMemcpyHostToDevice,
                                    r.stream);
        return hipMemcpyAsync(dst, r.arena->in.ptr + r.in_off, d * cs, hipMemcpyHostToDevice,
                              r.stream);
    }
    // This part's parity back to its caller (or the staging) on stream `q`.
    static hipError_t download(const PartReq& r, hipStream_t q) {
        const size_t p = r.codec->p, cs = r.at.stride;
        const uint8_t* src = r.dbuf + r.at.dev_parity;
        if (r.out_pinned && cs == r.L)  // straight into the caller's parity buffer
            return hipMemcpyAsync(r.parity_out, src, p * r.L, hipMemcpyDeviceToHost, q);
        if (r.out_pinned)  // p rows of L bytes out of the padded chunk stride
            return hipMemcpy2DAsync(r.parity_out, r.L, src, cs, r.L, p, hipMemcpyDeviceToHost, q);
        return hipMemcpyAsync(r.arena->out.ptr + r.at.out_off, src, p * cs, hipMemcpyDeviceToHost,
                              q);
    }
    // Each caller packs its own part: d rows of L bytes at the batch's row stride.  Nothing is
    // zeroed: the kernels read exactly L bytes per chunk.
    static void copy_in(PartReq& r) {
        if (!r.in_pinned) {
            const size_t d = r.codec->d, cs = r.at.stride;
            uint8_t* dst = r.arena->in.ptr + r.in_off;
            for (size_t j = 0; j < d; ++j) std::memcpy(dst + j * cs, r.data_buf + j * r.L, r.L);
        }
    }
    static int run(std::vector<PartReq*>& batch, Arena& a) {
        std::vector<plan::PartPlace> at;
        const plan::PartTotals tot = layout(batch, &at);
        if (!tot.mixed) return run_uniform(batch, a);
        g_mixed_batches.fetch_add(1, std::memory_order_relaxed);
        const int st = run_mixed(batch, a, at, tot);
        if (st != CEC_OK) {  // nothing of a failed batch stays in flight over the callers' buffers
            (void)hipStreamSynchronize(a.dev.stream);
            (void)hipGetLastError();
        }
        return st;
    }
    // Two or more chunk lengths: the split layout through ragged_launch.
    static int run_mixed(std::vector<PartReq*>& batch, Arena& a,
                         const std::vector<plan::PartPlace>& at, const plan::PartTotals& tot) {
        cec_codec* c = batch[0]->codec;
        const size_t B = batch.size();
        const bool per_part = any_pinned(batch);
        uint8_t* ddig = a.dev.dbuf;
        uint8_t* ddata = a.dev.dbuf + tot.dev_data;
        uint8_t* dpar = a.dev.dbuf + tot.dev_parity;
        hipStream_t s = a.dev.stream;
        std::vector<size_t> lens(B), doffs(B), poffs(B);
        for (size_t k = 0; k < B; ++k) {
            lens[k] = batch[k]->L;
            doffs[k] = at[k].dev_data - tot.dev_data;
            poffs[k] = at[k].dev_parity - tot.dev_parity;
        }
        CEC_TRY(split_check(c->d, c->p, ddata, doffs.data(), dpar, poffs.data(), lens.data(), B));
        if (!per_part) {  // the staging's offsets are the data region's
            HIP_TRY(hipMemcpyAsync(ddata, a.in.ptr, tot.in_bytes, hipMemcpyHostToDevice, s));
        } else {
            for (PartReq* r : batch) HIP_TRY(upload(*r));
        }
        CEC_TRY(ragged_launch(c, ddata, doffs.data(), dpar, poffs.data(), lens.data(), B, ddig, s));
        if (!per_part) {
            HIP_TRY(hipMemcpyAsync(a.out.ptr, dpar, tot.out_bytes, hipMemcpyDeviceToHost, s));
        } else {
            for (const PartReq* r : batch) HIP_TRY(download(*r, s));
        }
        HIP_TRY(hipMemcpyAsync(a.out.ptr + tot.out_bytes, ddig, tot.dig_bytes,
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return CEC_OK;
    }
    static int run_uniform(std::vector<PartReq*>& batch, Arena& a) {
        cec_codec* c = batch[0]->codec;
        const size_t d = c->d, p = c->p, t = d + p, B = batch.size();
        const size_t L = batch[0]->L, cs = batch[0]->at.stride;
        const bool per_part = any_pinned(batch);
        uint32_t* drec = nullptr;
        CEC_TRY(c->encode_record(&drec));
        uint8_t* ddig = a.dev.dbuf;
        uint8_t* dbase = a.dev.dbuf + round_up(B * t * 32, kChunkAlign);
        hipStream_t s = a.dev.stream;
        if (!per_part) {
            HIP_TRY(hipMemcpy2DAsync(dbase, t * cs, a.in.ptr, d * cs, d * cs, B,
                                     hipMemcpyHostToDevice, s));
        } else {
            for (PartReq* r : batch) HIP_TRY(upload(*r));  // pinned ones straight from the caller
        }
        // the parity of every part back to its caller (or the staging) on stream `q`
        auto parity_down = [&](hipStream_t q) -> int {
            if (!per_part) {
                HIP_TRY(hipMemcpy2DAsync(a.out.ptr, p * cs, dbase + d * cs, t * cs, p * cs, B,
                                         hipMemcpyDeviceToHost, q));
                return CEC_OK;
            }
            for (const PartReq* r : batch) HIP_TRY(download(*r, q));
            return CEC_OK;
        };
        // an error return after the side-stream download was queued must not leave it writing
        // into the callers' buffers: wait for it on every exit
        struct SideWait {
            hipStream_t q = nullptr;
            ~SideWait() {
                if (q) (void)hipStreamSynchronize(q);
            }
        } side_wait;
        // With separate kernels the encode's end is marked for the early parity download below.
        auto mark_encoded = [&]() -> int {
            if (!a.side) HIP_TRY(hipStreamCreateWithFlags(&a.side, hipStreamNonBlocking));
            if (!a.encoded) HIP_TRY(hipEventCreateWithFlags(&a.encoded, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(a.encoded, s));
            return CEC_OK;
        };
        bool split = false;  // device buffers from hipMalloc at 256-byte strides: always aligned
        CEC_TRY(encode_hash_steps(*c, drec, {dbase, t * cs, cs, B, L}, ddig, s, mark_encoded,
                                  &split));
        if (split) {
            // Parity down beside the SHA-256 chains (both only read the batch).  The leader
            // blocks on the encode's event, then queues the copy on the side stream.  A
            // device-side wait (the side stream waiting on the event) is deadlock-free too, since
            // the event is recorded before the wait is queued, and DESIGN.md §4.7's A/B put the
            // two within run-to-run spread; the host wait is the form with the longer record.
            HIP_TRY(hipEventSynchronize(a.encoded));
            side_wait.q = a.side;
            CEC_TRY(parity_down(a.side));
        } else {
            CEC_TRY(parity_down(s));
        }
        HIP_TRY(hipMemcpyAsync(a.out.ptr + batch[0]->item0, ddig, B * t * 32,
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (split) HIP_TRY(hipStreamSynchronize(a.side));
        return CEC_OK;
    }
    static void copy_out(PartReq& r) {
        const size_t d = r.codec->d, p = r.codec->p, t = d + p, cs = r.at.stride;
        if (!r.out_pinned) {
            const uint8_t* par = r.arena->out.ptr + r.at.out_off;
            for (size_t i = 0; i < p; ++i) std::memcpy(r.parity_out + i * r.L, par + i * cs, r.L);
        }
        std::memcpy(r.digests_out, r.arena->out.ptr + r.item0 + r.at.dig_off, t * 32);
    }
};

// ---- cec_part_read: one request = one part (its d+p slots, flags and expected digests) ----
// What the calls of one batch share: the round's place in the arena and the batch's arrays in
// cec_parts_read's form, filled by the callers (copy-in) and the launch.
struct ReadShared {
    Round round;
    std::vector<size_t> lens;
    std::vector<uint8_t> present, verified;
    std::vector<int> status;
};

struct ReadReq : ReqBase {
    cec_codec* codec = nullptr;
    uint8_t* const* shards = nullptr;   // d+p slots of L bytes
    size_t L = 0;
    const uint8_t* present = nullptr;   // d+p flags
    const uint8_t* expected = nullptr;  // (d+p)*32 bytes
    bool data_only = true;
    uint8_t* verified = nullptr;        // d+p flags, written
    int part_status = CEC_OK;           // CEC_OK or CEC_TOO_FEW_SHARDS_PRESENT
    std::shared_ptr<ReadShared> sh;
    CoalesceKey key() const { return {codec, data_only ? 1u : 0u, device}; }
};

// The steps of cec_parts_read's round (ragged.cpp, through capi_internal.hpp) with the staging
// and the collecting done by each caller for its own part.  Page-locked shard buffers are staged
// like pageable ones.
struct ReadImpl {
    static Counters& counters() { return g_read_counters; }
    static ArenaPool& arenas() { return ragged_arenas(); }
    // As cec_parts_read's rounds: the cap counts the (padded) data chunks.
    static size_t cap_bytes(const ReadReq& r) { return r.codec->d * ragged_stride(r.L); }
    static int prepare(std::vector<ReadReq*>& batch, Arena& a) {
        const cec_codec* c = batch[0]->codec;
        const size_t t = c->d + c->p, B = batch.size();
        auto sh = std::make_shared<ReadShared>();
        for (const ReadReq* r : batch) sh->lens.push_back(r->L);
        sh->present.resize(B * t);
        sh->verified.resize(B * t);
        sh->status.resize(B);
        CEC_TRY(reserve_round(a, c->d, t, sh->lens.data(), B, &sh->round));
        for (size_t k = 0; k < B; ++k) {
            batch[k]->arena = &a;
            batch[k]->slot = k;
            batch[k]->sh = sh;
        }
        return CEC_OK;
    }
    static void copy_in(ReadReq& r) {
        const size_t t = r.codec->d + r.codec->p;
        std::memcpy(r.sh->present.data() + r.slot * t, r.present, t);
        std::memcpy(r.arena->out.ptr + r.slot * t * 32, r.expected, t * 32);
        read_round_stage(r.sh->round, r.slot, t, r.L, r.shards, r.present);
    }
    static int run(std::vector<ReadReq*>& batch, Arena& a) {
        ReadReq& r = *batch[0];
        ReadShared& sh = *r.sh;
        const int st = read_round_launch(r.codec, a, sh.round, sh.lens.data(), batch.size(),
                                         sh.present.data(), r.data_only, sh.verified.data(),
                                         sh.status.data());
        if (st != CEC_OK && a.dev.stream) {  // nothing of a failed round stays in flight
            (void)hipStreamSynchronize(a.dev.stream);
            (void)hipGetLastError();
        }
        return st;
    }
    static void copy_out(ReadReq& r) {
        const size_t d = r.codec->d, t = d + r.codec->p;
        const uint8_t* ver = r.sh->verified.data() + r.slot * t;
        r.part_status = r.sh->status[r.slot];
        read_round_collect(r.sh->round, r.slot, d, t, r.L, r.shards, ver, r.part_status,
                           r.data_only);
        std::memcpy(r.verified, ver, t);
    }
};

Coalescer<ShaReq, ShaImpl> g_sha_queue;
Coalescer<PartReq, PartImpl> g_part_queue;
Coalescer<ReadReq, ReadImpl> g_read_queue;

int sha256_coalesced(const uint8_t* const* bufs, const size_t* lens, size_t n, uint8_t* out) {
    ShaReq r;
    CEC_TRY(current_device(&r.device));
    r.bufs = bufs;
    r.lens = lens;
    r.n = n;
    r.out = out;
    return g_sha_queue.submit(&r);
}

int part_encode_coalesced(cec_codec* c, const uint8_t* data_buf, size_t L, uint8_t* parity_out,
                          uint8_t* digests_out) {
    PartReq r;
    CEC_TRY(current_device(&r.device));
    r.codec = c;
    r.data_buf = data_buf;
    r.L = L;
    r.parity_out = parity_out;
    r.digests_out = digests_out;
    r.in_pinned = pinned_range(data_buf, c->d * L);
    r.out_pinned = pinned_range(parity_out, c->p * L);
    return g_part_queue.submit(&r);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Host-buffer API
// ------------------------------------------------------------------------------------------
extern "C" {

int cec_encode_sep(const cec_codec* cc, const uint8_t* const* data, const size_t* data_lens,
                   size_t n_data, uint8_t* const* parity, const size_t* parity_lens,
                   size_t n_parity) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    cec_codec* c = const_cast<cec_codec*>(cc);
    // check_piece_count!(data), check_piece_count!(parity)
    if (n_data < c->d) return CEC_TOO_FEW_DATA_SHARDS;
    if (n_data > c->d) return CEC_TOO_MANY_DATA_SHARDS;
    if (n_parity < c->p) return CEC_TOO_FEW_PARITY_SHARDS;
    if (n_parity > c->p) return CEC_TOO_MANY_PARITY_SHARDS;
    if (!data || !data_lens || !parity || !parity_lens) return CEC_ERR_INVALID_ARGUMENT;
    // check_slices!(multi => data, multi => parity)
    const size_t len = data_lens[0];
    if (len == 0) return CEC_EMPTY_SHARD;
    for (size_t j = 0; j < n_data; ++j)
        if (data_lens[j] != len) return CEC_INCORRECT_SHARD_SIZE;
    if (parity_lens[0] == 0) return CEC_EMPTY_SHARD;
    for (size_t i = 0; i < n_parity; ++i)
        if (parity_lens[i] != parity_lens[0]) return CEC_INCORRECT_SHARD_SIZE;
    if (parity_lens[0] != len) return CEC_INCORRECT_SHARD_SIZE;

    const size_t t = c->d + c->p, cs = round_up(len, kChunkAlign);
    uint32_t* drec = nullptr;
    CEC_TRY(c->encode_record(&drec));
    Lease<CtxPool> ctx;
    CEC_TRY(ctx.acquire(t * cs));
    for (size_t j = 0; j < c->d; ++j)
        HIP_TRY(hipMemcpyAsync(ctx->dbuf + j * cs, data[j], len, hipMemcpyHostToDevice,
                               ctx->stream));
    HIP_TRY(launch_encode(*c, drec, {ctx->dbuf, t * cs, cs, 1, len}, ctx->stream));
    for (size_t i = 0; i < c->p; ++i)
        HIP_TRY(hipMemcpyAsync(parity[i], ctx->dbuf + (c->d + i) * cs, len,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CEC_OK;
}

int cec_reconstruct(const cec_codec* c, uint8_t* const* shards, const size_t* lens,
                    uint8_t* present, size_t n) {
    return reconstruct_host(c, shards, lens, present, n, false);
}

int cec_reconstruct_data(const cec_codec* c, uint8_t* const* shards, const size_t* lens,
                         uint8_t* present, size_t n) {
    return reconstruct_host(c, shards, lens, present, n, true);
}

int cec_sha256_many(const uint8_t* const* bufs, const size_t* lens, size_t n, uint8_t* out) {
    if (n == 0) return CEC_OK;
    if (!bufs || !lens || !out) return CEC_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; ++i)
        if (lens[i] && !bufs[i]) return CEC_ERR_INVALID_ARGUMENT;
    return sha256_coalesced(bufs, lens, n, out);
}

int cec_sha256(const uint8_t* buf, size_t len, uint8_t* out32) {
    return cec_sha256_many(&buf, &len, 1, out32);
}

int cec_part_encode(const cec_codec* cc, const uint8_t* data_buf, size_t length,
                    uint8_t* parity_out, uint8_t* digests_out, size_t* chunksize) {
    if (!cc || !parity_out || !digests_out || !chunksize) return CEC_ERR_INVALID_ARGUMENT;
    if (length == 0) return CEC_EMPTY_SHARD;
    if (!data_buf) return CEC_ERR_INVALID_ARGUMENT;
    const size_t L = (length + cc->d - 1) / cc->d;
    CEC_TRY(part_encode_coalesced(const_cast<cec_codec*>(cc), data_buf, L, parity_out,
                                  digests_out));
    *chunksize = L;
    return CEC_OK;
}

int cec_part_read(const cec_codec* cc, uint8_t* const* shards, size_t chunk_len,
                  const uint8_t* present, const uint8_t* expected, int data_only,
                  uint8_t* verified) {
    if (!cc || !shards || !present || !expected || !verified) return CEC_ERR_INVALID_ARGUMENT;
    if (chunk_len == 0) return CEC_EMPTY_SHARD;
    const size_t d = cc->d, t = cc->d + cc->p;
    CEC_TRY(null_slot_rule("cec_part_read", shards, present, 1, d, t, data_only != 0));
    if (!ragged_stride(chunk_len) || ragged_stride(chunk_len) > SIZE_MAX / t)
        return CEC_ERR_INVALID_ARGUMENT;
    ReadReq r;
    CEC_TRY(current_device(&r.device));
    r.codec = const_cast<cec_codec*>(cc);
    r.shards = shards;
    r.L = chunk_len;
    r.present = present;
    r.expected = expected;
    r.data_only = data_only != 0;
    r.verified = verified;
    CEC_TRY(g_read_queue.submit(&r));
    return r.part_status;
}

void cec_coalesce_stats(uint64_t* calls, uint64_t* launches) {
    if (calls) *calls = g_write_counters.calls.load();
    if (launches) *launches = g_write_counters.launches.load();
}

void cec_coalesce_detail(uint64_t* part_mixed_batches, uint64_t* read_calls,
                         uint64_t* read_launches) {
    if (part_mixed_batches) *part_mixed_batches = g_mixed_batches.load();
    if (read_calls) *read_calls = g_read_counters.calls.load();
    if (read_launches) *read_launches = g_read_counters.launches.load();
}

size_t cec_release_cached(int device) { return CtxPool::get().trim(device); }

}  // extern "C"
