// capi_internal.hpp — what the pieces of the C-ABI (capi.cpp, its per-call tier percall.cpp and
// its ragged half ragged.cpp) share.  Not installed, not exported: everything here is defined
// once in capi.cpp unless it is inline.
#pragma once

#include "chunky_ec.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "gf256.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "percall_plan.hpp"

#pragma GCC visibility push(hidden)

#include "ragged_words.hpp"  // hidden like everything here: its templates export nothing
#include "scrub_words.hpp"
#include "segment_words.hpp"

namespace cec {

// The calling thread's last error text (cec_last_error).
void set_last_error(std::string msg);
const std::string& last_error();
int hip_fail(hipError_t e, const char* what);  // sets the last error; CEC_ERR_HIP / OUT_OF_MEMORY

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return cec::hip_fail(_e, #expr); \
    } while (0)

#define CEC_TRY(expr)              \
    do {                           \
        int _s = (expr);           \
        if (_s != CEC_OK) return _s; \
    } while (0)

int current_device(int* dev);

// Makes `device` current for a scope and restores the caller's device on every exit path.
class OnDevice {
   public:
    explicit OnDevice(int device) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != device) {
            err_ = hipSetDevice(device);
            switched_ = err_ == hipSuccess;
        }
    }
    ~OnDevice() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    hipError_t status() const { return err_; }

   private:
    int prev_ = 0;
    bool switched_ = false;
    hipError_t err_ = hipSuccess;
};

constexpr size_t kChunkAlign = 256;
inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline bool aligned16(const void* p, size_t a, size_t b) {
    return (reinterpret_cast<uintptr_t>(p) % 16 == 0) && (a % 16 == 0) && (b % 16 == 0);
}
inline bool aligned16(const cec_part_batch& b) {
    return aligned16(b.base, b.part_stride, b.chunk_stride);
}

inline size_t coalesce_max_bytes() { return knobs().coalesce_max_bytes; }

// A buffer of the scratch pool (capi.cpp ScratchPool): device memory with a page-locked host
// mirror, handed out again only once the event recorded after its last use has completed.
struct ScratchBuf {
    int device = 0;
    uint8_t* dev = nullptr;
    uint8_t* host = nullptr;  // page-locked mirror of the same size (null: a device-only buffer)
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool in_use = false;   // handed out, release not called yet
    bool pending = false;  // released: `done` marks the end of its last use
};

// One scratch buffer for the launches of one call: acquire, fill / upload, launch, and the
// destructor releases it on the stream those launches went to (error paths included).
class Scratch {
   public:
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch();
    // mirror false: device memory only (host() is null), for what never crosses the link
    int acquire(size_t bytes, hipStream_t s, bool mirror = true);
    uint8_t* dev() const { return buf_->dev; }
    uint8_t* host() const { return buf_->host; }

   private:
    ScratchBuf* buf_ = nullptr;
    hipStream_t stream_ = nullptr;
};

// Upload `words` into `sc` (acquired here) on stream s; *dptr = their device copy.
int upload_words(const std::vector<uint32_t>& words, hipStream_t s, Scratch& sc, uint32_t** dptr);

// Contexts a bounded per-device pool keeps alive between calls (percall.cpp CtxPool, capi.cpp
// SidePool).
constexpr size_t kMaxIdleCtx = 8;

// RAII lease of a pooled context on the current device.  Pool: Ctx; get(), the process-wide pool;
// take(device, args...), an idle or new context; prepare(ctx, args...), what a call needs of it
// (made on first use); give(ctx), back to the pool or destroyed.
template <typename Pool>
class Lease {
   public:
    Lease() = default;
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    ~Lease() { Pool::get().give(std::move(c_)); }
    template <typename... Args>
    int acquire(Args... args) {
        int dev = 0;
        CEC_TRY(current_device(&dev));
        c_ = Pool::get().take(dev, args...);
        return Pool::prepare(*c_, args...);
    }
    typename Pool::Ctx* operator->() { return c_.get(); }

   private:
    std::unique_ptr<typename Pool::Ctx> c_;
};

// A stream + a device staging buffer (leased from percall.cpp's CtxPool, or part of an Arena).
struct StageCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint8_t* dbuf = nullptr;
    size_t dcap = 0;
    void release_buffer() {
        if (dbuf) (void)hipFree(dbuf);
        dbuf = nullptr;
        dcap = 0;
    }
    void destroy() {  // on `device` (callers set it)
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        stream = nullptr;
        release_buffer();
    }
};

// Stream + device staging of at least device_bytes (grown, never shrunk while leased).
int ctx_reserve(StageCtx& c, size_t device_bytes);

// Pinned host staging, never shrunk.  Pinning costs ~0.35 s per GiB, so the first growth
// past 64 MiB goes straight to the batch cap (one pinning per process, not one per size step).
struct PinnedBuf {
    uint8_t* ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes, size_t cap_hint);
};

struct Arena {
    StageCtx dev;  // stream + device staging
    PinnedBuf in, out;
    // the parity comes back on a side stream as soon as the encode is done, beside the SHA-256
    // chains (profiles/r2_early_d2h/; made on first use; arenas live as long as the process)
    hipStream_t side = nullptr;
    hipEvent_t encoded = nullptr;
};

// A per-device free list of arenas: one per batch or call in flight, kept for the life of the
// process.
class ArenaPool {
   public:
    Arena* take(int device);
    void give(int device, Arena* a);

   private:
    std::mutex mu_;
    std::vector<std::unique_ptr<Arena>> all_;
    std::map<int, std::vector<Arena*>> free_;
};

// Erasure-pattern key: present bitset (<= 256 shards) + data_only.
struct PatternKey {
    std::array<uint64_t, 4> bits{};
    bool data_only = false;
    bool operator<(const PatternKey& o) const {
        if (bits != o.bits) return bits < o.bits;
        return data_only < o.data_only;
    }
};

// The host half of a batched reconstruct, shared by the uniform and the ragged layout: the parts
// that need a rebuild grouped by erasure pattern, one decode record per pattern, the patterns
// bucketed by output-row count, and per bucket the launch lists.
// words = [records...][launch lists: part_ids..., part_pat...].  Patterns of up to max_var_rows()
// rows (every RS(10,4) erasure set) share ONE launch that dispatches on each part's row count;
// wider patterns get a row-group launch per row count.
struct DecodePlan {
    struct Launch {
        uint32_t n_out;  // 0: per-part row counts (the shared launch)
        size_t ids;      // word offset of part_ids; part_pat follows at ids + count
        size_t count;
    };
    std::vector<uint32_t> words;
    std::vector<Launch> launches;  // empty: nothing to rebuild
    uint32_t var_rows = 0;         // the shared launch's widest pattern: its kernel's row class
};

void plan_decode(cec_codec* c, const uint8_t* present, size_t n_parts, bool data_only,
                 DecodePlan* plan);

// CEC_TOO_FEW_SHARDS_PRESENT when a part has some but fewer than d chunks present.
int check_present(size_t d, size_t t, const uint8_t* present, size_t n_parts);

// The shared launch's row class must cover every record it lists (the kernels skip a wider
// pattern without writing its chunks: kernels.hpp launch_rs_apply_var).
int check_row_class(const DecodePlan& plan, const DecodePlan::Launch& l, uint32_t n_rows,
                    const char* who);

// A loaded chunk is hashed unless the caller marked it CEC_PRESENT_VERIFIED (a read retry's
// chunks that an earlier pass already verified).
inline bool needs_hash(uint8_t f) { return f != 0 && f != CEC_PRESENT_VERIFIED; }

// From a verification's flags to the rebuild, for n_parts parts of t chunks.  Chunks an earlier
// pass verified (present == CEC_PRESENT_VERIFIED) are set in `verified`; part_status[k] = CEC_OK
// or, with fewer than d verified chunks, CEC_TOO_FEW_SHARDS_PRESENT (the reference's read returns
// such a part short / resilver reports it); *mask = the rebuild's present flags: a part's
// verified flags, or all ones (left alone) for a part that cannot be decoded and, with
// only_failed, for a part whose loaded chunks all verified (the uniform path's speculative pass
// rebuilt those; the ragged path has none and decodes every decodable part).  Returns whether
// any part kept its flags.
bool rebuild_mask(size_t d, size_t t, size_t n_parts, const uint8_t* present, uint8_t* verified,
                  int* part_status, bool only_failed, std::vector<uint8_t>* mask);

PatternKey make_key(const uint8_t* present, size_t t, bool data_only);

// ---- The launch steps over a uniform layout (cec_part_batch), one copy each. ----

// encode_sep of every part; rec = the codec's encode record on the current device.
hipError_t launch_encode(const cec_codec& c, const uint32_t* rec, const cec_part_batch& b,
                         hipStream_t s);

// The verify half of a strided SHA-256 launch (ShaParams: device pointers, all optional).
struct HashVerify {
    const uint8_t* present = nullptr;
    const uint8_t* expected = nullptr;
    uint8_t* ok = nullptr;
    const uint32_t* items = nullptr;  // the compacted item list, n_items of them
    uint32_t n_items = 0;
};
// SHA-256 of chunks [first_chunk, first_chunk + n_chunks) of every part: digests and/or verify.
hipError_t launch_hash(const cec_part_batch& b, size_t first_chunk, size_t n_chunks,
                       uint8_t* digests, const HashVerify& v, hipStream_t s);
// The list-mode ShaParams (device pointers): item i hashes lens[i] bytes at ptrs[i], i < items;
// order (null: every item) lists the `listed` items a launch hashes; digests and / or expected + ok.
ShaParams sha_list_params(const uint64_t* ptrs, const uint64_t* lens, size_t items,
                          const uint32_t* order, size_t listed, uint8_t* digests,
                          const uint8_t* expected = nullptr, uint8_t* ok = nullptr);

// One decode launch.  l: the listed parts of b, each with its own record in `words` (the shared
// launch when l->n_out == 0, n_rows its row class); null: every part of b through the n_rows
// rows of the one record at `words`.
hipError_t launch_decode(const cec_part_batch& b, size_t d, const uint32_t* words,
                         const DecodePlan::Launch* l, uint32_t n_rows, uint32_t lds_reserve,
                         hipStream_t s);

// Fused encode+hash kernel or encode kernel + SHA kernel for a batch of `chunks` chunks (d+p per
// part).  The fused kernel reads every byte once and wins when the SHA lanes fill the chip; a
// small batch leaves most SIMDs idle, and the split SHA kernel's lower per-chain latency (31 vs
// 42 ms per MiB) wins while the encode's extra pass is negligible.  CEC_FUSED (A/B knob): 0 =
// always separate, 1 = always fused where supported.
bool prefer_fused(size_t chunks);

// Encode + SHA-256 of all d+p chunks of every part (digests as in ShaParams): the fused kernel
// where it covers the shape, the layout is 16-byte aligned and prefer_fused says so; else the
// encode, after_encode() if given, then the SHA-256 launch, and *split (if given) = true.
int encode_hash_steps(const cec_codec& c, const uint32_t* rec, const cec_part_batch& b,
                      uint8_t* digests, hipStream_t s,
                      const std::function<int()>& after_encode = nullptr, bool* split = nullptr);

// ---- The ragged encode (ragged.cpp), as the parts pipeline (ragged_pipeline.cpp) shares it. ----

size_t ragged_stride(size_t chunk_len);  // cec_ragged_stride
// cec_split_layout behind its pointer checks.
int split_layout(size_t d, size_t p, const size_t* lens, size_t n, size_t* doffs, size_t* poffs,
                 size_t* data_bytes, size_t* parity_bytes);
// Every argument check of cec_encode_hash_split behind its pointer checks; no device use.
int split_check(size_t d, size_t p, const uint8_t* data, const size_t* doffs,
                const uint8_t* parity, const size_t* poffs, const size_t* lens, size_t n);
// Host-staged packing of n parts' data chunks into dst at offs (zero-padded), on up to 8 threads.
// seg_offs / seg_lens (null: whole chunks): only those columns of every chunk, as pieces of
// seg_lens[k] bytes.
void pack_parts(uint8_t* dst, const size_t* offs, size_t d, const uint8_t* const* bufs,
                const size_t* lengths, const size_t* chunk_lens, size_t n,
                const size_t* seg_offs = nullptr, const size_t* seg_lens = nullptr);
// The launches of a ragged encode + SHA-256 of checked arguments on s.  poffs null: parity behind
// each part's data (cec_encode_hash_ragged, `parity` unused); else the split layout.  hwords /
// dwords: page-locked and device room of plan::ragged_words_bytes for the words, which a caller that
// owns them must not reuse before the launches are done (null: a buffer of the scratch pool).
int ragged_launch(cec_codec* c, const uint8_t* data, const size_t* doffs, uint8_t* parity,
                  const size_t* poffs, const size_t* lens, size_t n, uint8_t* digests,
                  hipStream_t s, uint8_t* hwords = nullptr, uint8_t* dwords = nullptr);

// ---- The segmented encode (ragged.cpp), as the segment pipeline (segment_pipeline.cpp) shares it. ----

// Every check of cec_encode_hash_segments behind its null-pointer and zero-length checks; no
// device use.
int segments_check(size_t d, size_t p, const uint8_t* data, const size_t* doffs,
                   const uint8_t* parity, const size_t* poffs, const size_t* seg_lens, size_t n,
                   const uint32_t* slots, const uint8_t* flags, size_t n_slots);
// The launches of a checked segmented encode on s: the GF(2^8) kernel over the entries, then the
// resume launch.  hwords / dwords: page-locked and device room of plan::segment_words(t, n).bytes
// (null: a buffer of the scratch pool).  The resume launch waits for before_hash and after_hash is
// recorded behind it (either may be null).
int segments_launch(cec_codec* c, const uint8_t* data, const size_t* doffs, uint8_t* parity,
                    const size_t* poffs, const size_t* seg_lens, size_t n, const uint32_t* slots,
                    const uint8_t* flags, uint8_t* midstates, uint8_t* digests, hipStream_t s,
                    uint8_t* hwords = nullptr, uint8_t* dwords = nullptr,
                    hipEvent_t before_hash = nullptr, hipEvent_t after_hash = nullptr);

// ---- The segmented verification (ragged.cpp), as the scrub pipeline (scrub_pipeline.cpp) shares it. ----

// A caller's own staging for verify_segments_launch: page-locked and device memory of the same
// layout, [what the caller placed: the entries' bytes][at words_off, 16-byte aligned:
// plan::scrub_words(n)].
struct ScrubStage {
    uint8_t *h, *d;
    size_t words_off;
};
// The launch of a checked segmented verification on s: one upload, then the verifying resume
// launch.  stage null: words from the scratch pool, expected / ok the caller's device memory;
// else the words, the expected rows and the ok bytes are the staging's, and everything the staging
// holds up to the rows' end goes up in the one copy.  The launch waits for `before` and `after` is
// recorded behind it (either may be null).
int verify_segments_launch(const uint8_t* base, const size_t* offs, const size_t* seg_lens,
                           size_t n, const uint32_t* slots, const uint8_t* flags,
                           uint8_t* midstates, const uint8_t* expected, uint8_t* ok, hipStream_t s,
                           const ScrubStage* stage = nullptr, hipEvent_t before = nullptr,
                           hipEvent_t after = nullptr);

// ---- The ragged read (ragged.cpp), as the read pipeline (ragged_read_pipeline.cpp) shares it. ----

// cec_ragged_layout behind its pointer checks.
int ragged_layout(size_t t, const size_t* lens, size_t n, size_t* offs, size_t* total);
// (fills_slot, whether a read fills a slot that did not verify: percall_plan.hpp)
// The rule of cec_parts_read, cec_part_read and the parts reader for n parts' t slots each: a
// loaded chunk needs its bytes; a part that can be decoded (d or more chunks loaded) needs memory
// behind every slot the mode fills.  `who` opens the error text.
int null_slot_rule(const char* who, const uint8_t* const* shards, const uint8_t* present, size_t n,
                   size_t d, size_t t, bool data_only);
// The worst case of a packed return (cec_read_ragged_packed_async's bound on rebuilt_cap): the sum
// of rows * stride(L_k), rows = p, or min(p, d) under data_only.  Nonzero lengths.
int packed_worst_case(size_t d, size_t p, bool data_only, const size_t* lens, size_t n,
                      size_t* bytes);
// Host-staged packing of n parts' loaded chunks into dst at offs, on up to 8 threads.
void pack_loaded(uint8_t* dst, const size_t* offs, size_t t, const uint8_t* const* shards,
                 const size_t* chunk_lens, size_t n, const uint8_t* present);
// Copies of the byte ranges [first, second) (ascending, disjoint) between a pinned staging and a
// device arena that share their offsets, neighbours merged across small gaps.
// (Spans: percall_plan.hpp)
int copy_spans(uint8_t* stage, uint8_t* dbase, const Spans& spans, bool to_device, hipStream_t s);

// ---- One round of a host-staged read, as cec_parts_read (ragged.cpp) and cec_part_read's
// coalescer (percall.cpp) both run it: reserve, stage every part, launch, collect every part. ----

// The arenas of the host-staged ragged calls: one per call or batch in flight.
ArenaPool& ragged_arenas();

// One round's place in an arena: the packed layout of its n parts, `stage` (pinned) and `dbase`
// (device) sharing those offsets, and `dside`, device room for the round's n * t digests, with
// the arena's `out` as its pinned side.
struct Round {
    std::vector<size_t> offs;
    uint8_t *stage, *dside, *dbase;
    hipStream_t s;
};
int reserve_round(Arena& a, size_t d, size_t t, const size_t* chunk_lens, size_t n, Round* r);
// Stage: part k's loaded chunks (its t slots and flags, chunk length L) into the staging.
void read_round_stage(const Round& r, size_t k, size_t t, size_t L, uint8_t* const* shards,
                      const uint8_t* present);
// Launch: the n * t expected digests (already in a.out.ptr) and the loaded chunks up, the
// verification and the rebuild (the host-planned read, every (d, p)), the rebuilt chunks back into
// the staging, and the wait.  verified and part_status (host) are written.
int read_round_launch(cec_codec* c, Arena& a, const Round& r, const size_t* chunk_lens, size_t n,
                      const uint8_t* present, bool data_only, uint8_t* verified, int* part_status);
// Collect: part k's rebuilt chunks out of the staging into its slots.
void read_round_collect(const Round& r, size_t k, size_t d, size_t t, size_t L,
                        uint8_t* const* shards, const uint8_t* verified, int part_status,
                        bool data_only);

}  // namespace cec

#pragma GCC visibility pop

// The codec behind the C-ABI's handle: the coding matrix (one device copy per device, for the
// on-device decode planner), the encode record (one device copy per device) and the decode
// records by erasure pattern.
struct cec_codec {
    size_t d = 0, p = 0;
    cec::ByteMatrix m;             // (d+p) x d
    std::vector<uint32_t> enc;     // pattern record: parity rows over the d data chunks
    bool bs = false;               // parity rows = a compiled bit-sliced shape (bs_encode_matches)
    std::mutex mu;
    std::unordered_map<int, uint32_t*> dev_enc;  // encode record per device
    std::unordered_map<int, uint8_t*> dev_mat;   // coding matrix per device (matrix_device)
    // Decode records, least recently used first out once kDecCacheCap patterns are cached (every
    // 1..4-erasure pattern of RS(10,4), both modes, is 2 940).
    static constexpr size_t kDecCacheCap = 4096;
    using Record = std::shared_ptr<const std::vector<uint32_t>>;
    std::list<cec::PatternKey> dec_lru;  // front = most recent
    std::map<cec::PatternKey, std::pair<Record, std::list<cec::PatternKey>::iterator>> dec_cache;

    ~cec_codec() {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return;
        for (auto& kv : dev_enc) {
            if (hipSetDevice(kv.first) == hipSuccess) (void)hipFree(kv.second);
        }
        for (auto& kv : dev_mat) {
            if (hipSetDevice(kv.first) == hipSuccess) (void)hipFree(kv.second);
        }
        (void)hipSetDevice(cur);
    }

    // Device copy of `bytes` bytes at `src` on the current device, made on first use and kept in
    // `copies`.
    template <typename T>
    int device_copy(std::unordered_map<int, T*>& copies, const void* src, size_t bytes, T** out) {
        int dev = 0;
        CEC_TRY(cec::current_device(&dev));
        std::lock_guard<std::mutex> lk(mu);
        auto it = copies.find(dev);
        if (it != copies.end()) {
            *out = it->second;
            return CEC_OK;
        }
        T* ptr = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ptr), bytes));
        const hipError_t e = hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(ptr);
            return cec::hip_fail(e, "hipMemcpy (codec device copy)");
        }
        copies[dev] = ptr;
        *out = ptr;
        return CEC_OK;
    }

    // Device copy of the encode record on the current device.
    int encode_record(uint32_t** out) {
        return device_copy(dev_enc, enc.data(), enc.size() * sizeof(uint32_t), out);
    }

    // Device copy of the coding matrix ((d+p) x d bytes, row-major) on the current device.
    int matrix_device(uint8_t** out) { return device_copy(dev_mat, m.v.data(), m.v.size(), out); }

    // Decode record for a present set: inputs = first d present chunks (the crate's choice,
    // reconstruct_internal), outputs = missing data (+ missing parity unless data_only).
    // Missing data rows = rows of inv(M[valid]); missing parity rows = M[r] * inv(M[valid]),
    // i.e. the crate's "recompute parity from the rebuilt data" folded into one pass
    // (identical bytes: GF(2^8) arithmetic is exact).  Not exported, as before this header (its
    // key type then had internal linkage).
    __attribute__((visibility("hidden"))) Record decode_record(const cec::PatternKey& key) {
        using namespace cec;
        std::lock_guard<std::mutex> lk(mu);
        auto it = dec_cache.find(key);
        if (it != dec_cache.end()) {
            dec_lru.splice(dec_lru.begin(), dec_lru, it->second.second);
            return it->second.first;
        }
        const size_t t = d + p;
        std::vector<uint32_t> in_idx, out_idx;
        std::vector<size_t> miss_par;
        for (size_t i = 0; i < t; ++i) {
            const bool present = (key.bits[i / 64] >> (i % 64)) & 1;
            if (present) {
                if (in_idx.size() < d) in_idx.push_back(uint32_t(i));
            } else if (i < d) {
                out_idx.push_back(uint32_t(i));
            } else if (!key.data_only) {
                miss_par.push_back(i);
            }
        }
        for (size_t i : miss_par) out_idx.push_back(uint32_t(i));
        ByteMatrix sub(d, d), dec;
        for (size_t r = 0; r < d; ++r)
            for (size_t c = 0; c < d; ++c) sub.at(r, c) = m.at(in_idx[r], c);
        invert(sub, dec);  // any d rows of M are independent (distinct Vandermonde points)
        ByteMatrix rows(out_idx.size(), d);
        for (size_t k = 0; k < out_idx.size(); ++k) {
            const size_t o = out_idx[k];
            if (o < d) {
                for (size_t c = 0; c < d; ++c) rows.at(k, c) = dec.at(o, c);
            } else {
                const Gf256& g = Gf256::get();
                for (size_t c = 0; c < d; ++c) {
                    uint8_t acc = 0;
                    for (size_t q = 0; q < d; ++q) acc ^= g.mul(m.at(o, q), dec.at(q, c));
                    rows.at(k, c) = acc;
                }
            }
        }
        auto rec = std::make_shared<std::vector<uint32_t>>(pattern_words(d, out_idx.size()));
        write_pattern(rec->data(), d, in_idx, out_idx, rows);
        if (dec_cache.size() >= kDecCacheCap) {
            dec_cache.erase(dec_lru.back());
            dec_lru.pop_back();
        }
        dec_lru.push_front(key);
        dec_cache.emplace(key, std::make_pair(Record(rec), dec_lru.begin()));
        return rec;
    }

    size_t cached_patterns() {
        std::lock_guard<std::mutex> lk(mu);
        return dec_cache.size();
    }
};
