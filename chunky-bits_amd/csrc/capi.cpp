// capi.cpp — implementation of include/chunky_ec.h: the library and codec functions, the
// device-resident batch entry points, and the engine pieces every tier shares (error text,
// scratch pool, decode plan, the launch steps).  The host-buffer calls are in percall.cpp, the
// ragged batches in ragged.cpp.
//
// Host responsibilities only: argument checks in the crate's order, coding/decode matrices
// (tiny), erasure-pattern grouping, staging, and kernel launches.  Every shard byte is
// processed by the gfx950 kernels in kernels.hip; there is no CPU compute path.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>

using namespace cec;

namespace {

thread_local std::string g_last_error;

// ------------------------------------------------------------------------------------------
// Small per-launch device buffers (decode pattern records, verify item lists, flag arrays).
//
// Not hipMallocAsync / hipFreeAsync: with them, read and resilver batches came back with chunks
// the decode had not (re)written (round 2: the C++ mirror's batched verify/resilver and streamed
// reads, 4 of 4 runs).  tools/repro_free_async.hip shows why, with no engine code: on this
// ROCm, memory hipMallocAsync maps fresh (the default pool trimmed) is, on some boxes and every
// other allocation, zeroed AFTER the stream's first writes to it -- a kernel that filled it reads
// zeros on its later passes, and metadata words uploaded into it read as zeros (round 2's
// fork/join read shape loses whole outputs the same way, with the free queued behind the work
// or only after a sync).  hipMalloc'd memory never showed it (profiles/r3_repro/).
// Instead a process-wide pool of device buffers, each with a page-locked host mirror (device-only
// ones, for what never crosses the link, go without) and an event: a buffer is handed out only once the event recorded after its last use has
// completed, the words go up from the mirror (a truly asynchronous copy, no host lifetime to
// manage), and its release records the event on the stream of the work that used it.
// ------------------------------------------------------------------------------------------
class ScratchPool {
   public:
    using Buf = ScratchBuf;

    // A buffer of >= bytes on `device` whose last use has completed; with a page-locked mirror,
    // or (mirror false) one without.
    hipError_t acquire(int device, size_t bytes, bool mirror, Buf** out) {
        std::unique_lock<std::mutex> lk(mu_);
        Buf* best = nullptr;
        for (Buf* b : bufs_) {
            if (b->device != device || b->in_use || (b->host != nullptr) != mirror) continue;
            if (b->pending) {
                const hipError_t q = hipEventQuery(b->done);
                if (q == hipErrorNotReady) {
                    (void)hipGetLastError();
                    continue;
                }
                if (q != hipSuccess) {  // unknown state (e.g. its stream was destroyed): wait
                    (void)hipGetLastError();
                    if (hipEventSynchronize(b->done) != hipSuccess) {
                        (void)hipGetLastError();
                        continue;  // never reused
                    }
                }
                b->pending = false;
            }
            if (b->cap >= bytes && (!best || b->cap < best->cap)) best = b;
        }
        if (best) {
            best->in_use = true;
            *out = best;
            return hipSuccess;
        }
        // None free: a new buffer, made outside the lock (allocations are slow).
        lk.unlock();
        auto* b = new Buf();
        b->device = device;
        b->cap = std::max<size_t>(size_t(64) << 10, size_t(1) << (64 - __builtin_clzll(bytes | 1)));
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->dev), b->cap);
        if (e == hipSuccess && mirror)
            e = hipHostMalloc(reinterpret_cast<void**>(&b->host), b->cap, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b->done, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (b->dev) (void)hipFree(b->dev);
            if (b->host) (void)hipHostFree(b->host);
            delete b;
            return e;
        }
        b->in_use = true;
        lk.lock();
        bufs_.push_back(b);
        *out = b;
        return hipSuccess;
    }

    // The work that uses `b` has been queued on `s`: reusable once it completes.
    void release(Buf* b, hipStream_t s) {
        const hipError_t e = hipEventRecord(b->done, s);
        if (e != hipSuccess) {  // no marker: wait for the stream instead
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s);
            (void)hipGetLastError();
        }
        std::lock_guard<std::mutex> lk(mu_);
        b->pending = e == hipSuccess;
        b->in_use = false;
    }

   private:
    std::mutex mu_;
    std::vector<Buf*> bufs_;  // never freed: the pool lives as long as the process
};

ScratchPool& scratch_pool() {
    static auto* pool = new ScratchPool();
    return *pool;
}

// A kernel parameter block (ApplyParams, ShaParams, FusedParams, FillParams) over the layout b.
template <typename Params>
Params over(const cec_part_batch& b) {
    Params p{};
    p.base = b.base;
    p.part_stride = b.part_stride;
    p.chunk_stride = b.chunk_stride;
    p.len = b.chunk_len;
    p.n_parts = uint32_t(b.n_parts);
    return p;
}

}  // namespace

namespace cec {  // what capi_internal.hpp declares (described there)

PatternKey make_key(const uint8_t* present, size_t t, bool data_only) {
    PatternKey k;
    for (size_t i = 0; i < t; ++i)
        if (present[i]) k.bits[i / 64] |= uint64_t(1) << (i % 64);
    k.data_only = data_only;
    return k;
}

hipError_t launch_encode(const cec_codec& c, const uint32_t* rec, const cec_part_batch& b,
                         hipStream_t s) {
    ApplyParams a = over<ApplyParams>(b);
    a.pat = rec;
    a.d = uint32_t(c.d);
    a.n_rows = uint32_t(c.p);
    a.std_encode = c.bs ? 1u : 0u;
    return launch_rs_encode(a, aligned16(b), s);
}

hipError_t launch_hash(const cec_part_batch& b, size_t first_chunk, size_t n_chunks,
                       uint8_t* digests, const HashVerify& v, hipStream_t s) {
    ShaParams h = over<ShaParams>(b);
    h.first_chunk = uint32_t(first_chunk);
    h.n_chunks = uint32_t(n_chunks);
    h.digests = digests;
    h.present = v.present;
    h.expected = v.expected;
    h.ok = v.ok;
    h.items = v.items;
    h.n_items = v.n_items;
    return launch_sha256(h, aligned16(b), s);
}

ShaParams sha_list_params(const uint64_t* ptrs, const uint64_t* lens, size_t items,
                          const uint32_t* order, size_t listed, uint8_t* digests,
                          const uint8_t* expected, uint8_t* ok) {
    ShaParams h{};
    h.ptrs = ptrs;
    h.lens = lens;
    h.n_parts = uint32_t(items);
    h.n_chunks = 1;
    h.digests = digests;
    h.expected = expected;
    h.ok = ok;
    h.items = order;
    h.n_items = uint32_t(listed);
    return h;
}

hipError_t launch_decode(const cec_part_batch& b, size_t d, const uint32_t* words,
                         const DecodePlan::Launch* l, uint32_t n_rows, uint32_t lds_reserve,
                         hipStream_t s) {
    ApplyParams a = over<ApplyParams>(b);
    a.pat = words;
    a.d = uint32_t(d);
    a.n_rows = n_rows;
    if (l) {
        a.part_ids = words + l->ids;
        a.part_pat = words + l->ids + l->count;
        a.n_parts = uint32_t(l->count);
    }
    a.lds_reserve = lds_reserve;
    return l && !l->n_out ? launch_rs_apply_var(a, aligned16(b), s)
                          : launch_rs_apply(a, aligned16(b), s);
}

bool prefer_fused(size_t chunks) {
    const int f = knobs().fused;
    return f >= 0 ? f == 1 : !use_split(chunks);
}

int encode_hash_steps(const cec_codec& c, const uint32_t* rec, const cec_part_batch& b,
                      uint8_t* digests, hipStream_t s, const std::function<int()>& after_encode,
                      bool* split) {
    const size_t t = c.d + c.p;
    if (fused_covers(uint32_t(c.d), uint32_t(c.p), b.chunk_len) && aligned16(b) &&
        prefer_fused(b.n_parts * t)) {
        FusedParams f = over<FusedParams>(b);
        f.pat = rec;
        f.digests = digests;
        f.d = uint32_t(c.d);
        f.p = uint32_t(c.p);
        HIP_TRY(launch_encode_hash(f, true, s));
        return CEC_OK;
    }
    HIP_TRY(launch_encode(c, rec, b, s));
    if (after_encode) CEC_TRY(after_encode());
    HIP_TRY(launch_hash(b, 0, t, digests, {}, s));
    if (split) *split = true;
    return CEC_OK;
}

void set_last_error(std::string msg) { g_last_error = std::move(msg); }
const std::string& last_error() { return g_last_error; }

int hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? CEC_ERR_OUT_OF_MEMORY : CEC_ERR_HIP;
}

int current_device(int* dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_last_error = "no HIP device";
        return CEC_ERR_NO_DEVICE;
    }
    HIP_TRY(hipGetDevice(dev));
    return CEC_OK;
}

Scratch::~Scratch() {
    if (buf_) scratch_pool().release(buf_, stream_);
}

int Scratch::acquire(size_t bytes, hipStream_t s, bool mirror) {
    int dev = 0;
    CEC_TRY(current_device(&dev));
    HIP_TRY(scratch_pool().acquire(dev, bytes, mirror, &buf_));
    stream_ = s;
    return CEC_OK;
}

int upload_words(const std::vector<uint32_t>& words, hipStream_t s, Scratch& sc, uint32_t** dptr) {
    const size_t bytes = std::max<size_t>(words.size() * sizeof(uint32_t), 4);
    CEC_TRY(sc.acquire(bytes, s));
    std::memcpy(sc.host(), words.data(), words.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(sc.dev(), sc.host(), words.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, s));
    *dptr = reinterpret_cast<uint32_t*>(sc.dev());
    return CEC_OK;
}

int ctx_reserve(StageCtx& c, size_t device_bytes) {
    if (!c.stream) HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    if (c.dcap < device_bytes) {
        c.release_buffer();
        const size_t cap = round_up(std::max<size_t>(device_bytes, 1 << 20), 1 << 20);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c.dbuf), cap));
        c.dcap = cap;
    }
    return CEC_OK;
}

int PinnedBuf::reserve(size_t bytes, size_t cap_hint) {
    if (cap >= bytes) return CEC_OK;
    if (ptr) HIP_TRY(hipHostFree(ptr));
    ptr = nullptr;
    cap = 0;
    const size_t want =
        round_up(bytes <= (size_t(64) << 20) ? std::max(bytes, size_t(64) << 20)
                                             : std::max(bytes, cap_hint),
                 1 << 20);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ptr), want, hipHostMallocDefault));
    cap = want;
    return CEC_OK;
}

Arena* ArenaPool::take(int device) {
    std::lock_guard<std::mutex> lk(mu_);
    auto& v = free_[device];
    if (v.empty()) {
        all_.push_back(std::make_unique<Arena>());
        all_.back()->dev.device = device;
        return all_.back().get();
    }
    Arena* a = v.back();
    v.pop_back();
    return a;
}

void ArenaPool::give(int device, Arena* a) {
    std::lock_guard<std::mutex> lk(mu_);
    free_[device].push_back(a);
}

int check_present(size_t d, size_t t, const uint8_t* present, size_t n_parts) {
    for (size_t k = 0; k < n_parts; ++k) {
        size_t n_present = 0;
        for (size_t i = 0; i < t; ++i) n_present += present[k * t + i] ? 1 : 0;
        if (n_present != t && n_present < d) return CEC_TOO_FEW_SHARDS_PRESENT;
    }
    return CEC_OK;
}

int null_slot_rule(const char* who, const uint8_t* const* shards, const uint8_t* present, size_t n,
                   size_t d, size_t t, bool data_only) {
    for (size_t k = 0; k < n; ++k) {
        const size_t loaded = plan::loaded_count(present + k * t, t);
        for (size_t i = 0; i < t; ++i)
            if ((present[k * t + i] || plan::may_fill(i, d, loaded, data_only)) && !shards[k * t + i]) {
                set_last_error(std::string(who) + ": a chunk slot that is read or filled is NULL");
                return CEC_ERR_INVALID_ARGUMENT;
            }
    }
    return CEC_OK;
}

void plan_decode(cec_codec* c, const uint8_t* present, size_t n_parts, bool data_only,
                 DecodePlan* plan) {
    const size_t t = c->d + c->p;
    // Group parts by pattern; bucket patterns by output-row count.
    std::map<PatternKey, std::pair<uint32_t, std::vector<uint32_t>>> groups;  // key -> (n_out, parts)
    for (size_t k = 0; k < n_parts; ++k) {
        const uint8_t* pr = present + k * t;
        size_t n_present = 0;
        for (size_t i = 0; i < t; ++i) n_present += pr[i] ? 1 : 0;
        if (n_present == t) continue;
        PatternKey key = make_key(pr, t, data_only);
        auto& g = groups[key];
        g.second.push_back(uint32_t(k));
    }
    std::vector<uint32_t>& words = plan->words;
    std::map<uint32_t, std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> buckets;
    for (auto& kv : groups) {
        auto rec = c->decode_record(kv.first);
        const uint32_t n_out = (*rec)[0];
        if (n_out == 0) continue;  // data_only: only parity missing, nothing to do
        if (n_out <= max_var_rows()) plan->var_rows = std::max(plan->var_rows, n_out);
        const uint32_t off = uint32_t(words.size());
        words.insert(words.end(), rec->begin(), rec->end());
        auto& bk = buckets[n_out <= max_var_rows() ? 0u : n_out];  // 0 = the shared launch
        for (uint32_t part : kv.second.second) {
            bk.first.push_back(part);
            bk.second.push_back(off);
        }
    }
    for (auto& kv : buckets) {
        plan->launches.push_back({kv.first, words.size(), kv.second.first.size()});
        words.insert(words.end(), kv.second.first.begin(), kv.second.first.end());
        words.insert(words.end(), kv.second.second.begin(), kv.second.second.end());
    }
}

int check_row_class(const DecodePlan& plan, const DecodePlan::Launch& l, uint32_t n_rows,
                    const char* who) {
    const uint32_t* pat_off = plan.words.data() + l.ids + l.count;
    for (size_t q = 0; q < l.count; ++q)
        if (plan.words[pat_off[q]] == 0 || plan.words[pat_off[q]] > n_rows) {
            g_last_error = std::string(who) + ": a listed pattern is wider than its launch";
            return CEC_ERR_INVALID_ARGUMENT;
        }
    return CEC_OK;
}

bool rebuild_mask(size_t d, size_t t, size_t n_parts, const uint8_t* present, uint8_t* verified,
                  int* part_status, bool only_failed, std::vector<uint8_t>* mask) {
    const size_t n = n_parts * t;
    for (size_t i = 0; i < n; ++i)  // verified by an earlier pass: trusted, not hashed again
        if (present[i] == CEC_PRESENT_VERIFIED) verified[i] = 1;
    mask->assign(n, uint8_t(1));
    bool any = false;
    for (size_t k = 0; k < n_parts; ++k) {
        size_t good = 0;
        bool bad = false;
        for (size_t i = 0; i < t; ++i) {
            good += verified[k * t + i] ? 1 : 0;
            bad |= present[k * t + i] && !verified[k * t + i];
        }
        part_status[k] = good >= d ? CEC_OK : CEC_TOO_FEW_SHARDS_PRESENT;
        if (good >= d && (bad || !only_failed)) {
            std::copy(verified + k * t, verified + (k + 1) * t, mask->begin() + k * t);
            any = true;
        }
    }
    return any;
}

}  // namespace cec

namespace {

int batch_ok(const cec_part_batch* b) {
    if (!b || !b->base) return CEC_ERR_INVALID_ARGUMENT;
    return CEC_OK;
}

// cec_reconstruct_batch with each decode block reserving lds_reserve bytes of LDS (see
// ApplyParams::lds_reserve).
int reconstruct_batch(const cec_codec* cc, const cec_part_batch* b, const uint8_t* present,
                      int data_only, void* stream, uint32_t lds_reserve) {
    if (!cc || !present) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(batch_ok(b));
    if (b->n_parts == 0) return CEC_OK;
    if (b->chunk_len == 0) return CEC_EMPTY_SHARD;
    if (b->n_parts > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    cec_codec* c = const_cast<cec_codec*>(cc);
    const size_t d = c->d, t = c->d + c->p;
    // Validate every part before launching anything.
    CEC_TRY(check_present(d, t, present, b->n_parts));
    DecodePlan plan;
    plan_decode(c, present, b->n_parts, data_only != 0, &plan);
    if (plan.launches.empty()) return CEC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* dwords = nullptr;
    Scratch scratch;  // released on s behind the launches below
    CEC_TRY(upload_words(plan.words, s, scratch, &dwords));
    int status = CEC_OK;
    for (size_t i = 0; i < plan.launches.size() && status == CEC_OK; ++i) {
        const DecodePlan::Launch& l = plan.launches[i];
        const uint32_t n_rows = l.n_out ? l.n_out : plan.var_rows;
        if (!l.n_out) CEC_TRY(check_row_class(plan, l, n_rows, "reconstruct_batch"));
        hipError_t e = launch_decode(*b, d, dwords, &l, n_rows, lds_reserve, s);
        if (e != hipSuccess) status = hip_fail(e, "launch_rs_apply");
    }
    return status;
}

// Side stream of the speculative decode in cec_read_batch / cec_resilver_batch, with the
// fork/join events that order it against the caller's stream: leased per call from a bounded
// per-device pool (see percall.cpp's CtxPool for why not thread_local).
struct SideCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    void destroy() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        stream = nullptr;
        fork = join = nullptr;
    }
};

class SidePool {
   public:
    using Ctx = SideCtx;
    static SidePool& get() {
        static SidePool* pool = new SidePool();  // leaked: see CtxPool::get()
        return *pool;
    }
    static int prepare(SideCtx& c) {
        if (!c.stream) HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        if (!c.fork) HIP_TRY(hipEventCreateWithFlags(&c.fork, hipEventDisableTiming));
        if (!c.join) HIP_TRY(hipEventCreateWithFlags(&c.join, hipEventDisableTiming));
        return CEC_OK;
    }
    std::unique_ptr<SideCtx> take(int device) {
        std::lock_guard<std::mutex> lk(mu_);
        auto& v = idle_[device];
        if (v.empty()) {
            auto c = std::make_unique<SideCtx>();
            c->device = device;
            return c;
        }
        auto c = std::move(v.back());
        v.pop_back();
        return c;
    }
    void give(std::unique_ptr<SideCtx> c) {
        if (!c) return;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto& v = idle_[c->device];
            if (v.size() < kMaxIdleCtx) {
                v.push_back(std::move(c));
                return;
            }
        }
        c->destroy();
    }

   private:
    std::mutex mu_;
    std::map<int, std::vector<std::unique_ptr<SideCtx>>> idle_;
};

// LDS each speculative-decode block reserves.  100 KiB keeps decode blocks off the CUs holding
// SHA workgroups (>= 64 KiB each) and runs one per free CU: a low-intensity decode spread under
// the SHA chains.  Measured on the c3r read (4 096 parts, RS(10,4), d loaded,
// profiles/r1y_c3r_summary.md): 43.2 ms vs 45.3 (65 KiB: two per free CU) vs 46.5 (none: decode
// everywhere, done in 17 ms, but the SHA chains slow from 42.6 to 46.4 ms beside it) vs 53.0 ms
// without speculation.
constexpr uint32_t kDecodeLds = 100u * 1024u;

// DataVerifier::verify of the loaded chunks (present_host[k*t + i] != 0) of a batch: ok[item] =
// digest matches (ok of the others is left as is).  The loaded chunks are packed into a
// compacted item list, so a read with d of d+p chunks loaded runs d/(d+p) of the waves of a
// strided launch with skipped lanes (a SHA wave costs the same with idle lanes), which leaves
// SIMDs free for the decode running beside it.
int verify_loaded(const cec_part_batch* b, size_t t, const uint8_t* present_host,
                  const uint8_t* expected, uint8_t* ok, hipStream_t s) {
    const size_t n = b->n_parts * t;
    std::vector<uint32_t> items;
    items.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (needs_hash(present_host[i])) items.push_back(uint32_t(i));
    if (items.empty()) return CEC_OK;
    const uint32_t n_items = uint32_t(items.size());
    uint32_t* ditems = nullptr;
    Scratch sc;  // released on s behind the verification launch
    CEC_TRY(upload_words(items, s, sc, &ditems));
    hipError_t e = launch_hash(*b, 0, t, nullptr, {nullptr, expected, ok, ditems, n_items}, s);
    if (e != hipSuccess) return hip_fail(e, "launch_sha256 (verify)");
    return CEC_OK;
}

// Shared body of cec_read_batch / cec_resilver_batch.  The result is the reference's: rebuild
// from the first d VERIFIED chunks of each part (file_part.rs:98-128 keeps only chunks whose hash
// matched).  The decode does not wait for the verdict: the pattern is known from the loaded
// flags, so it runs speculatively from the first d LOADED chunks on a side stream, concurrently
// with the SHA-256 verification (which leaves 384 of 1 024 SIMDs idle on a 4 096-part RS(10,4)
// read: 40 960 chains = 640 waves).  Both only read the loaded chunks and the decode writes only
// chunks that were not loaded, so they do not race.  When every loaded chunk verifies (the
// common case) the speculative result is the final one; a part with a loaded chunk that failed
// is decoded again from its verified chunks, which rewrites every chunk the first pass wrote.
int verify_then_reconstruct(const cec_codec* c, const cec_part_batch* b,
                            const uint8_t* present_host, const uint8_t* expected,
                            uint8_t* verified_host, int* part_status, bool data_only,
                            hipStream_t s) {
    if (!c || !present_host || !expected || !verified_host || !part_status)
        return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(batch_ok(b));
    if (b->n_parts == 0) return CEC_OK;
    if (b->chunk_len == 0) return CEC_EMPTY_SHARD;
    const size_t d = c->d, t = c->d + c->p, n = b->n_parts * t;
    if (n > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    Scratch ok_buf;  // device verification flags, released on s behind the readback
    CEC_TRY(ok_buf.acquire(n, s));
    uint8_t* ok = ok_buf.dev();
    HIP_TRY(hipMemsetAsync(ok, 0, n, s));
    // Fork point: the caller's work on s so far (the chunks).  The side stream waits for it and
    // s later waits for the side stream's join, each on an event recorded before the wait is
    // queued: safe in shared in-order hardware queues (the rule of the coalescer's early parity
    // download above).
    Lease<SidePool> side;
    CEC_TRY(side.acquire());
    HIP_TRY(hipEventRecord(side->fork, s));
    // Verification goes first so its long-lived workgroups claim their CUs (one or two per CU)
    // before the decode's blocks take the CUs left free.
    int st = verify_loaded(b, t, present_host, expected, ok, s);
    if (st == CEC_OK) {
        // Parts with fewer than d loaded chunks cannot be decoded: left out (mask all ones).
        std::vector<uint8_t> spec(present_host, present_host + n);
        for (size_t k = 0; k < b->n_parts; ++k) {
            const size_t loaded =
                size_t(std::count_if(spec.begin() + k * t, spec.begin() + (k + 1) * t,
                                     [](uint8_t f) { return f != 0; }));
            if (loaded < d) std::fill(spec.begin() + k * t, spec.begin() + (k + 1) * t, uint8_t(1));
        }
        hipError_t e = hipStreamWaitEvent(side->stream, side->fork, 0);
        if (e != hipSuccess) st = hip_fail(e, "speculative decode fork");
        if (st == CEC_OK)
            st = reconstruct_batch(c, b, spec.data(), data_only ? 1 : 0, side->stream,
                                   kDecodeLds);
        if (st == CEC_OK) {
            e = hipEventRecord(side->join, side->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, side->join, 0);
            if (e != hipSuccess) st = hip_fail(e, "speculative decode join");
        }
        // On failure nothing joins the side stream: let what it launched finish before the
        // caller gets its buffers back.
        if (st != CEC_OK) (void)hipStreamSynchronize(side->stream);
    }
    if (st == CEC_OK) {
        hipError_t e = hipMemcpyAsync(verified_host, ok, n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) st = hip_fail(e, "verify readback");
    }
    if (st != CEC_OK) return st;
    // Decode again the parts whose loaded chunks did not all verify.
    std::vector<uint8_t> pres;
    if (!rebuild_mask(d, t, b->n_parts, present_host, verified_host, part_status, true, &pres))
        return CEC_OK;
    return reconstruct_batch(c, b, pres.data(), data_only ? 1 : 0, s, 0);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Library
// ------------------------------------------------------------------------------------------
extern "C" {

int cec_abi_version(void) { return CEC_ABI_VERSION; }

const char* cec_build_info(void) {
    return "chunky_ec gfx950 ab_tools=0";
}

const char* cec_status_name(int s) {
    switch (s) {
        case CEC_OK: return "Ok";
        case CEC_TOO_FEW_SHARDS: return "TooFewShards";
        case CEC_TOO_MANY_SHARDS: return "TooManyShards";
        case CEC_TOO_FEW_DATA_SHARDS: return "TooFewDataShards";
        case CEC_TOO_MANY_DATA_SHARDS: return "TooManyDataShards";
        case CEC_TOO_FEW_PARITY_SHARDS: return "TooFewParityShards";
        case CEC_TOO_MANY_PARITY_SHARDS: return "TooManyParityShards";
        case CEC_TOO_FEW_BUFFER_SHARDS: return "TooFewBufferShards";
        case CEC_TOO_MANY_BUFFER_SHARDS: return "TooManyBufferShards";
        case CEC_INCORRECT_SHARD_SIZE: return "IncorrectShardSize";
        case CEC_TOO_FEW_SHARDS_PRESENT: return "TooFewShardsPresent";
        case CEC_EMPTY_SHARD: return "EmptyShard";
        case CEC_INVALID_SHARD_FLAGS: return "InvalidShardFlags";
        case CEC_INVALID_INDEX: return "InvalidIndex";
        case CEC_ERR_INVALID_ARGUMENT: return "InvalidArgument";
        case CEC_ERR_HIP: return "HipError";
        case CEC_ERR_NO_DEVICE: return "NoDevice";
        case CEC_ERR_OUT_OF_MEMORY: return "OutOfMemory";
        default: return "Unknown";
    }
}

const char* cec_last_error(void) { return g_last_error.c_str(); }

int cec_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------
// Codec
// ------------------------------------------------------------------------------------------

int cec_codec_new(size_t d, size_t p, cec_codec** out) {
    if (!out) return CEC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    // ReedSolomon::new order of checks.
    if (d == 0) return CEC_TOO_FEW_DATA_SHARDS;
    if (p == 0) return CEC_TOO_FEW_PARITY_SHARDS;
    if (d + p > 256) return CEC_TOO_MANY_SHARDS;
    auto c = std::make_unique<cec_codec>();
    c->d = d;
    c->p = p;
    c->m = build_coding_matrix(d, p);
    ByteMatrix rows(p, d);
    std::vector<uint32_t> in_idx(d), out_idx(p);
    for (size_t j = 0; j < d; ++j) in_idx[j] = uint32_t(j);
    for (size_t i = 0; i < p; ++i) {
        out_idx[i] = uint32_t(d + i);
        for (size_t j = 0; j < d; ++j) rows.at(i, j) = c->m.at(d + i, j);
    }
    c->enc.resize(pattern_words(d, p));
    write_pattern(c->enc.data(), d, in_idx, out_idx, rows);
    c->bs = d <= 0xFFFFFFFFull && p <= 0xFFFFFFFFull &&
            bs_encode_matches(uint32_t(d), uint32_t(p), rows.v.data());
    *out = c.release();
    return CEC_OK;
}

void cec_codec_free(cec_codec* c) { delete c; }
size_t cec_codec_data_shards(const cec_codec* c) { return c ? c->d : 0; }
size_t cec_codec_parity_shards(const cec_codec* c) { return c ? c->p : 0; }
size_t cec_codec_total_shards(const cec_codec* c) { return c ? c->d + c->p : 0; }
size_t cec_codec_cached_patterns(const cec_codec* c) {
    return c ? const_cast<cec_codec*>(c)->cached_patterns() : 0;
}

int cec_codec_matrix(const cec_codec* c, uint8_t* out, size_t out_len) {
    if (!c || !out || out_len < c->m.v.size()) return CEC_ERR_INVALID_ARGUMENT;
    std::memcpy(out, c->m.v.data(), c->m.v.size());
    return CEC_OK;
}

// ------------------------------------------------------------------------------------------
// Device-resident batches (the host-buffer API is percall.cpp)
// ------------------------------------------------------------------------------------------

int cec_encode_batch(const cec_codec* cc, const cec_part_batch* b, void* stream) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(batch_ok(b));
    if (b->n_parts == 0) return CEC_OK;
    if (b->chunk_len == 0) return CEC_EMPTY_SHARD;
    if (b->n_parts > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    cec_codec* c = const_cast<cec_codec*>(cc);
    uint32_t* drec = nullptr;
    CEC_TRY(c->encode_record(&drec));
    HIP_TRY(launch_encode(*c, drec, *b, static_cast<hipStream_t>(stream)));
    return CEC_OK;
}

int cec_sha256_batch(const cec_part_batch* b, size_t first_chunk, size_t n_chunks,
                     uint8_t* digests, void* stream) {
    CEC_TRY(batch_ok(b));
    if (!digests) return CEC_ERR_INVALID_ARGUMENT;
    if (b->n_parts == 0 || n_chunks == 0) return CEC_OK;
    if (b->n_parts * n_chunks > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    HIP_TRY(launch_hash(*b, first_chunk, n_chunks, digests, {}, static_cast<hipStream_t>(stream)));
    return CEC_OK;
}

int cec_encode_hash_batch(const cec_codec* cc, const cec_part_batch* b, uint8_t* digests,
                          void* stream) {
    if (!cc || !digests) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(batch_ok(b));
    if (b->n_parts == 0) return CEC_OK;
    if (b->chunk_len == 0) return CEC_EMPTY_SHARD;
    if (b->n_parts * (cc->d + cc->p) > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    cec_codec* c = const_cast<cec_codec*>(cc);
    uint32_t* drec = nullptr;
    CEC_TRY(c->encode_record(&drec));
    return encode_hash_steps(*c, drec, *b, digests, static_cast<hipStream_t>(stream));
}

int cec_reconstruct_batch(const cec_codec* c, const cec_part_batch* b, const uint8_t* present,
                          int data_only, void* stream) {
    return reconstruct_batch(c, b, present, data_only, stream, 0);
}

int cec_verify_batch(const cec_part_batch* b, size_t first_chunk, size_t n_chunks,
                     const uint8_t* present, const uint8_t* expected, uint8_t* ok, void* stream) {
    CEC_TRY(batch_ok(b));
    if (!expected || !ok) return CEC_ERR_INVALID_ARGUMENT;
    if (b->n_parts == 0 || n_chunks == 0) return CEC_OK;
    if (b->n_parts * n_chunks > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    HIP_TRY(launch_hash(*b, first_chunk, n_chunks, nullptr, {present, expected, ok},
                        static_cast<hipStream_t>(stream)));
    return CEC_OK;
}

int cec_read_batch(const cec_codec* c, const cec_part_batch* b, const uint8_t* present,
                   const uint8_t* expected, uint8_t* verified, int* part_status, void* stream) {
    return verify_then_reconstruct(c, b, present, expected, verified, part_status, true,
                                   static_cast<hipStream_t>(stream));
}

int cec_resilver_batch(const cec_codec* c, const cec_part_batch* b, const uint8_t* present,
                       const uint8_t* expected, uint8_t* verified, int* part_status,
                       void* stream) {
    return verify_then_reconstruct(c, b, present, expected, verified, part_status, false,
                                   static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------
// Utilities
// ------------------------------------------------------------------------------------------

int cec_fill_synthetic(const cec_part_batch* b, size_t n_chunks, uint64_t seed, void* stream) {
    CEC_TRY(batch_ok(b));
    if (b->n_parts > 0xFFFFFFFFull || n_chunks > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    FillParams f = over<FillParams>(*b);
    f.seed = seed;
    f.n_chunks = uint32_t(n_chunks);
    HIP_TRY(launch_fill(f, static_cast<hipStream_t>(stream)));
    return CEC_OK;
}

uint8_t cec_synth_byte(uint64_t seed, uint64_t part, uint64_t chunk, uint64_t offset) {
    return synth_byte(seed, part, chunk, offset);
}

}  // extern "C"
