// ragged.cpp — the ragged half of include/chunky_ec.h: parts of different chunk lengths in one
// launch sequence (cec_encode_hash_ragged, cec_encode_hash_split, cec_encode_hash_segments, which
// takes parts as column segments and resumes their SHA-256 chains, cec_reconstruct_ragged,
// cec_verify_ragged, cec_verify_segments (copies as segments, their chains resumed and ended by a
// verdict), cec_read_ragged, cec_resilver_ragged and their _async forms, which plan the
// decode on the device and never wait, cec_read_ragged_packed_async among them) and the host-staged calls on top of
// them (cec_parts_encode, cec_parts_read, cec_parts_verify).  Part k's chunk i lies at
// base + off[k] + i * stride(L_k), stride = L rounded up to 16; the split layout keeps the parity
// chunks in a region of their own.  Host work only; every step of the path has one home here
// (the ragged write pipeline, ragged_pipeline.cpp, and the ragged read pipeline,
// ragged_read_pipeline.cpp, take their steps from here through capi_internal.hpp).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "capi_internal.hpp"

using namespace cec;

using plan::kRaggedAlign;

// L rounded up to 16; 0 when that overflows (and for an empty chunk, which every caller refuses
// before it asks).
size_t cec::ragged_stride(size_t L) { return plan::stride16(L); }

// The packed layout: part k+1 directly behind part k (the rule itself: percall_plan.hpp).
int cec::ragged_layout(size_t t, const size_t* lens, size_t n, size_t* offs, size_t* total) {
    const int st = plan::packed_layout(t, lens, n, offs, total);
    return st == 0 ? CEC_OK : st == 1 ? CEC_EMPTY_SHARD : CEC_ERR_INVALID_ARGUMENT;
}

namespace {

// Every argument check of a ragged layout of t chunks per part (no device use), the bound on the
// launch's work units among them.
int ragged_check(size_t t, const uint8_t* base, const size_t* offs, const size_t* lens, size_t n) {
    size_t items = 0;  // SHA-256 items are 32-bit (checked before the arrays are walked)
    if (__builtin_mul_overflow(n, t, &items) || items > 0xFFFFFFFFull)
        return CEC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < n; ++k)
        if (lens[k] == 0) return CEC_EMPTY_SHARD;
    if (reinterpret_cast<uintptr_t>(base) % kRaggedAlign) return CEC_ERR_INVALID_ARGUMENT;
    const uint64_t unit = ragged_unit_bytes(), max_units = ragged_max_units();
    uint64_t total = 0;
    size_t end = 0;  // first byte behind the parts so far
    for (size_t k = 0; k < n; ++k) {
        const size_t cs = ragged_stride(lens[k]);
        size_t span = 0;
        if (offs[k] % kRaggedAlign || offs[k] < end) return CEC_ERR_INVALID_ARGUMENT;
        if (!cs || __builtin_mul_overflow(t, cs, &span) || span > SIZE_MAX - offs[k])
            return CEC_ERR_INVALID_ARGUMENT;
        end = offs[k] + span;
        total += (uint64_t(lens[k] - 1)) / unit + 1;
        if (total > max_units) return CEC_ERR_INVALID_ARGUMENT;  // never a silent wrap
    }
    return CEC_OK;
}

}  // namespace

// Every argument check of a split layout (no device use): each region by ragged_check's rules,
// d chunks per part in the data region and p in the parity region, the SHA-256 items of both
// together, and the two regions' byte ranges apart.
int cec::split_check(size_t d, size_t p, const uint8_t* data, const size_t* doffs,
                     const uint8_t* parity, const size_t* poffs, const size_t* lens, size_t n) {
    size_t items = 0;
    if (__builtin_mul_overflow(n, d + p, &items) || items > 0xFFFFFFFFull)
        return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(ragged_check(d, data, doffs, lens, n));
    CEC_TRY(ragged_check(p, parity, poffs, lens, n));
    if (n == 0) return CEC_OK;
    const size_t cs = ragged_stride(lens[n - 1]);
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(data), p0 = reinterpret_cast<uintptr_t>(parity);
    uintptr_t d_lo = 0, d_hi = 0, p_lo = 0, p_hi = 0;
    if (__builtin_add_overflow(d0, doffs[0], &d_lo) ||
        __builtin_add_overflow(d0, doffs[n - 1] + d * cs, &d_hi) ||
        __builtin_add_overflow(p0, poffs[0], &p_lo) ||
        __builtin_add_overflow(p0, poffs[n - 1] + p * cs, &p_hi))
        return CEC_ERR_INVALID_ARGUMENT;
    if (d_lo < p_hi && p_lo < d_hi) {
        set_last_error("split layout: the data and the parity region overlap");
        return CEC_ERR_INVALID_ARGUMENT;
    }
    return CEC_OK;
}

namespace {

// Ragged encode launch sequences since load, by path (cec_ragged_stats).
std::atomic<uint64_t> g_fused_seqs{0}, g_two_pass_seqs{0};

// What an unset CEC_RAGGED_FUSED selects for a launch too large for the split SHA-256 kernel:
// fused only if its worst repeat is below two-pass's best repeat in all three configurations of
// tools/small_files_bench.py --device.  One run (profiles/small_files/device_fused.log), event
// intervals of three alternating repeats, two-pass against fused:
//   4096 x RS(10,4) x 64 KiB, uniform lengths      3.75-3.93 ms   3.33-3.45 ms   fused wins
//   4096 files of 1 KiB-4 MiB as RS(3,2) parts    42.58-42.68 ms 42.24-42.29 ms  fused wins
//   the same files as RS(10,4) parts              17.76-17.83 ms 19.26-19.27 ms  two-pass wins
// The mixed batches are bound by the SHA-256 chain of their longest chunk, which the fused
// workgroup's lane waves walk with a barrier per step beside the encoders: not in all three, so
// two-pass stays and the kernel is reached through the knob.
constexpr bool kRaggedFusedDefault = false;

// Whether a ragged encode of n parts of these (checked) lengths takes the fused kernel
// (fused_kernels.hip encode_hash_ragged_kernel) or the GF(2^8) launch and the SHA-256 list launch.
// As prefer_fused for the uniform batches: CEC_RAGGED_FUSED 0 / 1 forces one, else two-pass while
// the SHA-256 launch would take the split kernel (lower latency per chain), and above that what
// the measurement says.  Shapes the fused kernel does not cover take two passes whatever the knob.
bool ragged_prefers_fused(size_t d, size_t p, const size_t* lens, size_t n) {
    if (!fused_ragged_covers(uint32_t(d), uint32_t(p))) return false;
    for (size_t k = 0; k < n; ++k)
        if (lens[k] >> 39) return false;  // the kernel's 32-bit step count
    const int f = knobs().ragged_fused;
    return f >= 0 ? f == 1 : !use_split(n * (d + p)) && kRaggedFusedDefault;
}

// The RaggedParams of a launch over n_parts listed parts, in the order of its fields (kernels.hpp):
// device pointers; part_pat null: every part uses the record at pat.
RaggedParams ragged_params(uint8_t* base, const uint32_t* pat, const uint32_t* units,
                           const uint32_t* parts, const uint32_t* part_pat, size_t n_parts,
                           uint32_t total_units, size_t d, size_t n_rows, bool split = false) {
    return {base, pat, units, parts, part_pat, uint32_t(n_parts), total_units, uint32_t(d),
            uint32_t(n_rows), split ? 1u : 0u};
}

}  // namespace

// The launches of a checked ragged encode on `s`: one upload of the per-part words, then the
// fused kernel (part order, part records), or the GF(2^8) kernel and the SHA-256 kernel (the
// SHA-256 list, the part records).  The host arrays are copied into the words' page-locked side
// before this returns.  Part k's data chunks lie at data + doffs[k]; its parity chunks behind
// them (poffs null: the layout of cec_ragged_layout, records without a displacement) or at
// parity + poffs[k] (the split layout).
int cec::ragged_launch(cec_codec* c, const uint8_t* data, const size_t* doffs, uint8_t* parity,
                       const size_t* poffs, const size_t* lens, size_t n, uint8_t* digests,
                       hipStream_t s, uint8_t* hwords, uint8_t* dwords) {
    const size_t d = c->d, t = c->d + c->p, items = n * t;
    uint32_t* drec = nullptr;
    CEC_TRY(c->encode_record(&drec));
    const bool fused = ragged_prefers_fused(d, c->p, lens, n);
    const plan::EncodeWords w = plan::encode_words(t, n, fused, poffs != nullptr);
    Scratch sc;  // the words of a caller that has none: released on s behind the launches below
    if (!hwords) {
        CEC_TRY(sc.acquire(w.bytes, s));
        hwords = sc.host();
        dwords = sc.dev();
    }
    const plan::View v{hwords, dwords};
    // where part k's parity chunk 0 lies, less where today's layout has it
    std::vector<uint64_t> disp(poffs ? n : 0);
    for (size_t k = 0; k < disp.size(); ++k)
        disp[k] = (reinterpret_cast<uint64_t>(parity) + poffs[k]) -
                  (reinterpret_cast<uint64_t>(data) + doffs[k] + d * ragged_stride(lens[k]));
    if (fused)
        plan::length_order(lens, n, v.host(w.list.order));
    else
        plan::sha_list(
            lens, n, t, [](size_t) { return true; },
            [&](size_t k, size_t i, size_t cs) {
                return i < d || !poffs ? data + doffs[k] + i * cs
                                       : parity + poffs[k] + (i - d) * cs;
            },
            v.host(w.list.ptrs), v.host(w.list.lens), v.host(w.list.order));
    const uint32_t total_units = plan::part_records(
        ragged_unit_bytes(), doffs, lens, nullptr, n, fused ? nullptr : v.host(w.units),
        v.host(w.parts), poffs ? disp.data() : nullptr);
    HIP_TRY(hipMemcpyAsync(dwords, hwords, w.bytes, hipMemcpyHostToDevice, s));
    if (fused) {
        FusedRaggedParams f{};
        f.base = const_cast<uint8_t*>(data);  // split: only read
        f.pat = drec;
        f.order = v.dev(w.list.order);
        f.parts = v.dev(w.parts);
        f.digests = digests;
        f.n_parts = uint32_t(n);
        f.d = uint32_t(d);
        f.p = uint32_t(c->p);
        f.split = poffs ? 1u : 0u;
        HIP_TRY(launch_encode_hash_ragged(f, s));
        g_fused_seqs.fetch_add(1, std::memory_order_relaxed);
        return CEC_OK;
    }
    const RaggedParams a =
        ragged_params(const_cast<uint8_t*>(data) /* split: only read */, drec, v.dev(w.units),
                      v.dev(w.parts), nullptr, n, total_units, d, c->p, poffs != nullptr);
    HIP_TRY(launch_rs_encode_ragged(a, s));
    const ShaParams h = sha_list_params(v.dev(w.list.ptrs), v.dev(w.list.lens), items,
                                        v.dev(w.list.order), items, digests);
    HIP_TRY(launch_sha256(h, true, s));
    g_two_pass_seqs.fetch_add(1, std::memory_order_relaxed);
    return CEC_OK;
}

// The checks of cec_encode_hash_segments behind its null-pointer and zero-length checks (no
// device use): the split layout's rules over the segment lengths, then the segment rules.
int cec::segments_check(size_t d, size_t p, const uint8_t* data, const size_t* doffs,
                        const uint8_t* parity, const size_t* poffs, const size_t* seg_lens,
                        size_t n, const uint32_t* slots, const uint8_t* flags, size_t n_slots) {
    CEC_TRY(split_check(d, p, data, doffs, parity, poffs, seg_lens, n));
    switch (plan::segment_rules(seg_lens, slots, flags, n, n_slots)) {
        case 0: break;
        case 1:
            set_last_error("segments: an entry that is not CEC_SEG_LAST has a length that is no "
                           "multiple of 64");
            return CEC_ERR_INVALID_ARGUMENT;
        case 2:
            set_last_error("segments: a state slot is not below n_state_slots");
            return CEC_ERR_INVALID_ARGUMENT;
        default:
            set_last_error("segments: two entries of one call name the same state slot");
            return CEC_ERR_INVALID_ARGUMENT;
    }
    for (size_t k = 0; k < n; ++k)  // the kernel's record index is 32-bit
        if (plan::touches_record(flags[k]) && (uint64_t(slots[k]) + 1) * (d + p) > 0xFFFFFFFFull)
            return CEC_ERR_INVALID_ARGUMENT;
    return CEC_OK;
}

// The launches of a checked segmented encode on `s`: one upload of the words, the GF(2^8) kernel
// over the entries (to it a segment is a part of chunk length seg_lens[k] in the split layout) and
// the resume launch over the n * (d + p) chunk segments (sha256_resume_kernels.hip).  Always two
// passes.  The host arrays are copied into the words' page-locked side before this returns.
// before_hash (null: none): an event the resume launch waits for; after_hash (null: none): an
// event recorded behind it, for a caller that orders the chains of successive calls across streams.
int cec::segments_launch(cec_codec* c, const uint8_t* data, const size_t* doffs, uint8_t* parity,
                         const size_t* poffs, const size_t* seg_lens, size_t n,
                         const uint32_t* slots, const uint8_t* flags, uint8_t* midstates,
                         uint8_t* digests, hipStream_t s, uint8_t* hwords, uint8_t* dwords,
                         hipEvent_t before_hash, hipEvent_t after_hash) {
    const size_t d = c->d, t = c->d + c->p, items = n * t;
    uint32_t* drec = nullptr;
    CEC_TRY(c->encode_record(&drec));
    const plan::SegmentWords w = plan::segment_words(t, n);
    Scratch sc;  // the words of a caller that has none: released on s behind the launches below
    if (!hwords) {
        CEC_TRY(sc.acquire(w.bytes, s));
        hwords = sc.host();
        dwords = sc.dev();
    }
    const plan::View v{hwords, dwords};
    std::vector<uint64_t> disp(n);  // where entry k's parity piece 0 lies, behind its data pieces
    for (size_t k = 0; k < n; ++k)
        disp[k] = (reinterpret_cast<uint64_t>(parity) + poffs[k]) -
                  (reinterpret_cast<uint64_t>(data) + doffs[k] + d * ragged_stride(seg_lens[k]));
    const plan::ShaListWords& l = w.resume.list;
    plan::sha_list(
        seg_lens, n, t, [](size_t) { return true; },
        [&](size_t k, size_t i, size_t cs) {
            return i < d ? data + doffs[k] + i * cs : parity + poffs[k] + (i - d) * cs;
        },
        v.host(l.ptrs), v.host(l.lens), v.host(l.order));
    plan::resume_items(slots, flags, n, t, v.host(w.resume.record), v.host(w.resume.flags));
    const uint32_t total_units =
        plan::part_records(ragged_unit_bytes(), doffs, seg_lens, nullptr, n, v.host(w.units),
                           v.host(w.parts), disp.data());
    HIP_TRY(hipMemcpyAsync(dwords, hwords, w.bytes, hipMemcpyHostToDevice, s));
    const RaggedParams a = ragged_params(const_cast<uint8_t*>(data) /* split: only read */, drec,
                                         v.dev(w.units), v.dev(w.parts), nullptr, n, total_units,
                                         d, c->p, true);
    HIP_TRY(launch_rs_encode_ragged(a, s));
    if (before_hash) HIP_TRY(hipStreamWaitEvent(s, before_hash, 0));
    const ShaResumeParams h{v.dev(l.ptrs),         v.dev(l.lens),         v.dev(l.order),
                            v.dev(w.resume.record), v.dev(w.resume.flags), midstates,
                            digests,               uint32_t(items)};
    HIP_TRY(launch_sha256_resume(h, s));
    if (after_hash) HIP_TRY(hipEventRecord(after_hash, s));
    return CEC_OK;
}

// The launch of a checked segmented verification on `s`: the words filled (scrub_words.hpp), one
// upload, then the verifying resume launch over the n entries (sha256_resume_kernels.hip).  Entry k
// is seg_lens[k] bytes at base + offs[k].  The host arrays are copied into the words' page-locked
// side before this returns.  Without `stage` the words take a buffer of the scratch pool, only the
// list goes up, and expected / ok are the caller's device rows and bytes.  With it the words lie
// at stage->words_off of the caller's page-locked and device staging, whose bytes from 0 to the
// end of the words' expected rows go up in the one copy (the caller filled the data before them
// and the rows), and expected / ok are the words' own regions.  before / after: as segments_launch.
int cec::verify_segments_launch(const uint8_t* base, const size_t* offs, const size_t* seg_lens,
                                size_t n, const uint32_t* slots, const uint8_t* flags,
                                uint8_t* midstates, const uint8_t* expected, uint8_t* ok,
                                hipStream_t s, const ScrubStage* stage, hipEvent_t before,
                                hipEvent_t after) {
    const plan::ScrubWords w = plan::scrub_words(n);
    Scratch sc;  // the words of a caller that has none: released on s behind the launch below
    if (!stage) CEC_TRY(sc.acquire(w.resume.bytes, s));
    const plan::View v = stage ? plan::View{stage->h + stage->words_off, stage->d + stage->words_off}
                               : plan::View{sc.host(), sc.dev()};
    plan::scrub_fill(reinterpret_cast<uint64_t>(base), offs, seg_lens, n, slots, flags, w.resume, v);
    if (stage) {
        HIP_TRY(hipMemcpyAsync(stage->d, stage->h, stage->words_off + w.up_bytes,
                               hipMemcpyHostToDevice, s));
        expected = v.dev(w.expected)->b;
        ok = v.dev(w.ok);
    } else {
        HIP_TRY(hipMemcpyAsync(v.d, v.h, w.resume.bytes, hipMemcpyHostToDevice, s));
    }
    if (before) HIP_TRY(hipStreamWaitEvent(s, before, 0));
    const plan::ShaListWords& l = w.resume.list;
    const ShaVerifyResumeParams h{v.dev(l.ptrs),          v.dev(l.lens),         v.dev(l.order),
                                  v.dev(w.resume.record), v.dev(w.resume.flags), midstates,
                                  expected,               ok,                    uint32_t(n)};
    const hipError_t e = launch_sha256_resume_verify(h, s);
    if (e != hipSuccess) return hip_fail(e, "launch_sha256_resume_verify");
    if (after) HIP_TRY(hipEventRecord(after, s));
    return CEC_OK;
}

namespace {

// The launches of cec_reconstruct_ragged for a checked layout (ragged_check) and checked flags
// (check_present), on `s`.  Only the parts the plan lists reach the device: per launch the part
// records of its listed parts, behind the plan's words in one scratch buffer whose page-locked
// mirror holds the copy of the host arrays.
int reconstruct_ragged(cec_codec* c, uint8_t* base, const size_t* offs, const size_t* lens,
                       size_t n, const uint8_t* present, bool data_only, hipStream_t s) {
    DecodePlan plan;
    plan_decode(c, present, n, data_only, &plan);
    if (plan.launches.empty()) return CEC_OK;
    for (const auto& l : plan.launches)
        if (!l.n_out) CEC_TRY(check_row_class(plan, l, plan.var_rows, "reconstruct_ragged"));
    const plan::ReconWords w = plan::recon_words(plan.words.size(), plan.launches);
    Scratch sc;  // released on s behind the launches below
    CEC_TRY(sc.acquire(w.bytes, s));
    const plan::View v{sc.host(), sc.dev()};
    std::memcpy(v.host(w.plan), plan.words.data(), plan.words.size() * sizeof(uint32_t));
    const uint32_t* dplan = v.dev(w.plan);
    std::vector<RaggedParams> params;
    for (size_t i = 0; i < plan.launches.size(); ++i) {
        const auto& l = plan.launches[i];
        const uint32_t total_units =
            plan::part_records(ragged_unit_bytes(), offs, lens, plan.words.data() + l.ids, l.count,
                               v.host(w.units[i]), v.host(w.parts[i]));
        params.push_back(ragged_params(base, dplan, v.dev(w.units[i]), v.dev(w.parts[i]),
                                       dplan + l.ids + l.count, l.count, total_units, c->d,
                                       l.n_out ? l.n_out : plan.var_rows));
    }
    HIP_TRY(hipMemcpyAsync(sc.dev(), sc.host(), w.bytes, hipMemcpyHostToDevice, s));
    for (size_t i = 0; i < params.size(); ++i) {
        const hipError_t e = plan.launches[i].n_out ? launch_rs_encode_ragged(params[i], s)
                                                    : launch_rs_reconstruct_ragged(params[i], s);
        if (e != hipSuccess) return hip_fail(e, "launch_rs_reconstruct_ragged");
    }
    return CEC_OK;
}

// The queued half of a ragged verification for a checked layout of t chunks per part: on `s` one
// upload, the memset of ok[items] (device) and the SHA-256 list launch in verify mode over the
// chunks that need hashing (present null: all of them; ok and expected indexed by k*t+i).
// v: page-locked and device room for the list `w` (of n * t items, at the start of both) and,
// directly behind it, `tail` bytes of the caller's own words, filled on the page-locked side
// before the call, which go up in the same copy.  tail == 0: only the listed part of the list goes
// up, and nothing when nothing is hashed.  No wait; nothing of `base` is written.
int verify_launch(const uint8_t* base, const size_t* offs, const size_t* lens, size_t n, size_t t,
                  const uint8_t* present, const uint8_t* expected, const plan::ShaListWords& w,
                  const plan::View& v, size_t tail, uint8_t* ok, hipStream_t s) {
    const size_t items = n * t;
    const size_t hashed = plan::sha_list(
        lens, n, t, [&](size_t item) { return !present || needs_hash(present[item]); },
        [&](size_t k, size_t i, size_t cs) { return base + offs[k] + i * cs; }, v.host(w.ptrs),
        v.host(w.lens), v.host(w.order));
    const size_t up = tail ? w.bytes + tail : w.up_bytes(hashed);
    if (up) HIP_TRY(hipMemcpyAsync(v.d, v.h, up, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(ok, 0, items, s));
    if (hashed) {
        const ShaParams h = sha_list_params(v.dev(w.ptrs), v.dev(w.lens), items, v.dev(w.order),
                                            hashed, nullptr, expected, ok);
        const hipError_t e = launch_sha256(h, true, s);
        if (e != hipSuccess) return hip_fail(e, "launch_sha256 (ragged verify)");
    }
    return CEC_OK;
}

// The verification half of the ragged read side for a checked layout of t chunks per part: on `s`
// the verification (verify_launch), then the readback of the flags, the one wait.
// `verified` is written once they are back: the kernel's flag for a hashed chunk, 1 for a
// CEC_PRESENT_VERIFIED one, 0 for an absent one.  Nothing of `base` is written.
int verify_ragged(const uint8_t* base, const size_t* offs, const size_t* lens, size_t n, size_t t,
                  const uint8_t* present, const uint8_t* expected, uint8_t* verified,
                  hipStream_t s) {
    const size_t items = n * t;
    const plan::VerifyWords w = plan::verify_words(items);
    Scratch sc;  // released on s behind the readback
    CEC_TRY(sc.acquire(w.bytes, s));
    const plan::View v{sc.host(), sc.dev()};
    CEC_TRY(verify_launch(base, offs, lens, n, t, present, expected, w.list, v, 0, v.dev(w.ok), s));
    // the flags come back through the mirror, behind the words that went up
    HIP_TRY(hipMemcpyAsync(v.host(w.ok), v.dev(w.ok), items, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(verified, v.host(w.ok), items);
    for (size_t i = 0; present && i < items; ++i)  // trusted, not hashed
        if (present[i] == CEC_PRESENT_VERIFIED) verified[i] = 1;
    return CEC_OK;
}

// Shared body of cec_read_ragged / cec_resilver_ragged for a checked layout: the verification
// (verify_ragged), then on `s` the rebuild of every decodable part from its first d verified
// chunks.
// No speculative decode beside the verification: the form without the wait (read_ragged_async)
// has nothing for one to hide.
int read_ragged(cec_codec* c, uint8_t* base, const size_t* offs, const size_t* lens, size_t n,
                const uint8_t* present, const uint8_t* expected, uint8_t* verified,
                int* part_status, bool data_only, hipStream_t s) {
    const size_t d = c->d, t = c->d + c->p;
    CEC_TRY(verify_ragged(base, offs, lens, n, t, present, expected, verified, s));
    std::vector<uint8_t> pres;
    rebuild_mask(d, t, n, present, verified, part_status, false, &pres);
    return reconstruct_ragged(c, base, offs, lens, n, pres.data(), data_only, s);
}

// cec_read_ragged_async / cec_resilver_ragged_async calls since load, by who planned the decode
// (cec_ragged_read_stats).
std::atomic<uint64_t> g_device_planned{0}, g_host_planned{0};

// The most rows a part's record can have: every chunk the mode fills may be missing, but never
// more than p of them in a part that decodes.
inline size_t plan_rows(size_t d, size_t p, bool data_only) { return data_only ? std::min(p, d) : p; }

// The packed return of read_ragged_async: a device region of `cap` bytes and the host array of
// n + 1 byte offsets into it.
struct PackedReturn {
    uint8_t* rebuilt;
    size_t cap;
    size_t* offsets;
};

// Whether read_ragged_async covers a batch: the planner kernel's shape, and record offsets
// (k * slot words) that fit the reconstruct launch's 32-bit part_pat.
bool device_plan_covers(size_t d, size_t p, size_t n, bool data_only) {
    if (d > 0xFFFFFFFFull || p > 0xFFFFFFFFull || !decode_plan_covers(uint32_t(d), uint32_t(p)))
        return false;
    return n <= 0xFFFFFFFFull / pattern_words(d, plan_rows(d, p, data_only));
}

}  // namespace

// The most a packed return of these (checked, nonzero) chunk lengths can hold: every part with
// all its rows rebuilt.
int cec::packed_worst_case(size_t d, size_t p, bool data_only, const size_t* lens, size_t n,
                           size_t* bytes) {
    const size_t rows = plan_rows(d, p, data_only);
    size_t acc = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t cs = ragged_stride(lens[k]);
        size_t b = 0;
        if (!cs || __builtin_mul_overflow(rows, cs, &b) || __builtin_add_overflow(acc, b, &acc))
            return CEC_ERR_INVALID_ARGUMENT;
    }
    *bytes = acc;
    return CEC_OK;
}

namespace {

// cec_read_ragged_async / cec_resilver_ragged_async for a checked layout and a covered shape
// (device_plan_covers): verification, decode plan and rebuild of every part queued on `s`, then
// the copies of the flags and the statuses into the caller's (host) memory.  Nothing here waits
// for the device: the plan is built there (plan_kernels.hip), one record per part in the part's
// own slot, and rs_reconstruct_ragged_kernel runs over ALL parts, writing nothing for a part
// whose record is empty (not decodable, or nothing to rebuild).
// present, offs and lens are copied into the words' page-locked side before this returns.  Both
// scratch buffers are released on `s` behind the last copy.
// ret (null: none of this): the packed return.  Behind the rebuild, the scan of the records'
// returns and the gather of every rebuilt chunk into ret->rebuilt (plan_kernels.hip
// launch_return_plan), then the copy of the n + 1 offsets into ret->offsets (host).  The caller
// checked the region against packed_worst_case.
int read_ragged_async(cec_codec* c, uint8_t* base, const size_t* offs, const size_t* lens, size_t n,
                      const uint8_t* present, const uint8_t* expected, uint8_t* verified,
                      int* part_status, bool data_only, hipStream_t s,
                      const PackedReturn* ret = nullptr) {
    const size_t d = c->d, t = c->d + c->p, items = n * t;
    const size_t rows = plan_rows(d, c->p, data_only), slot = pattern_words(d, rows);
    // what goes up, in one copy, and what stays on the device
    const plan::ReadUpWords wu = plan::read_up_words(t, n);
    const plan::ReadDevWords wd = plan::read_dev_words(t, n, slot, ret != nullptr);
    // every allocation before anything is queued
    Scratch up, dv;
    CEC_TRY(up.acquire(wu.bytes, s));
    CEC_TRY(dv.acquire(wd.bytes, s, false));
    uint8_t* dmat = nullptr;
    CEC_TRY(c->matrix_device(&dmat));

    const plan::View vu{up.host(), up.dev()}, vd{nullptr, dv.dev()};
    const uint32_t total_units = plan::part_records(ragged_unit_bytes(), offs, lens, nullptr, n,
                                                    vu.host(wu.units), vu.host(wu.parts));
    uint32_t* part_pat = vu.host(wu.part_pat);
    for (size_t k = 0; k < n; ++k) part_pat[k] = uint32_t(k * slot);
    std::memcpy(vu.host(wu.present), present, items);
    uint8_t* ok = vd.dev(wd.ok);
    CEC_TRY(verify_launch(base, offs, lens, n, t, present, expected, wu.list, vu,
                          wu.bytes - wu.list.bytes, ok, s));
    PlanParams pl{};
    pl.present = vu.dev(wu.present);
    pl.ok = ok;
    pl.matrix = dmat;
    pl.verified = vd.dev(wd.verified);
    pl.part_status = vd.dev(wd.status);
    pl.records = vd.dev(wd.records);
    pl.n_parts = uint32_t(n);
    pl.d = uint32_t(d);
    pl.p = uint32_t(c->p);
    pl.slot_words = uint32_t(slot);
    pl.max_rows = uint32_t(rows);
    pl.data_only = data_only ? 1u : 0u;
    hipError_t e = launch_decode_plan(pl, s);
    if (e != hipSuccess) return hip_fail(e, "launch_decode_plan");
    const RaggedParams a = ragged_params(base, pl.records, vu.dev(wu.units), vu.dev(wu.parts),
                                         vu.dev(wu.part_pat), n, total_units, d, rows);
    e = launch_rs_reconstruct_ragged(a, s);
    if (e != hipSuccess) return hip_fail(e, "launch_rs_reconstruct_ragged (device plan)");
    uint64_t* ret_off = ret ? vd.dev(wd.ret_off) : nullptr;
    if (ret) {
        ReturnParams r{};
        r.base = base;
        r.records = pl.records;
        r.units = a.units;
        r.parts = a.parts;
        r.ret_off = ret_off;
        r.rebuilt = ret->rebuilt;
        r.unit_bytes = ragged_unit_bytes();
        r.n_parts = uint32_t(n);
        r.total_units = total_units;
        r.d = uint32_t(d);
        r.t = uint32_t(t);
        r.slot_words = uint32_t(slot);
        r.max_rows = uint32_t(rows);
        e = launch_return_plan(r, s);
        if (e != hipSuccess) return hip_fail(e, "launch_return_plan");
    }
    HIP_TRY(hipMemcpyAsync(verified, pl.verified, items, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(part_status, pl.part_status, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (ret) {
        static_assert(sizeof(size_t) == sizeof(uint64_t), "the offsets are copied as they are");
        HIP_TRY(hipMemcpyAsync(ret->offsets, ret_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    return CEC_OK;
}

// Every check of cec_read_ragged / cec_resilver_ragged and their _async forms, then the work.
// async: the no-wait path where the planner kernel covers the shape; other shapes take the
// synchronous path inside the same call (its wait is verify_ragged's).
int read_ragged_checked(const cec_codec* cc, uint8_t* base, const size_t* offs, const size_t* lens,
                        size_t n, const uint8_t* present, const uint8_t* expected,
                        uint8_t* verified, int* part_status, bool data_only, void* stream,
                        bool async = false, const PackedReturn* ret = nullptr) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n == 0) {  // a batch of nothing returns nothing
        if (ret && ret->offsets) ret->offsets[0] = 0;
        return CEC_OK;
    }
    if (!base || !offs || !lens || !present || !expected || !verified || !part_status)
        return CEC_ERR_INVALID_ARGUMENT;
    if (ret && (!ret->rebuilt || !ret->offsets)) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(ragged_check(cc->d + cc->p, base, offs, lens, n));
    if (ret) {  // the packed return's own checks, still before any device use
        size_t worst = 0;
        if (reinterpret_cast<uintptr_t>(ret->rebuilt) % kRaggedAlign) return CEC_ERR_INVALID_ARGUMENT;
        if (!device_plan_covers(cc->d, cc->p, n, data_only)) {
            set_last_error("cec_read_ragged_packed_async: the device planner covers d <= 32 and "
                           "p <= 8; use cec_read_ragged_async for this shape");
            return CEC_ERR_INVALID_ARGUMENT;
        }
        CEC_TRY(packed_worst_case(cc->d, cc->p, data_only, lens, n, &worst));
        if (ret->cap < worst) {
            set_last_error("cec_read_ragged_packed_async: rebuilt_cap is below the batch's worst "
                           "case, the sum of rows * cec_ragged_stride(L_k)");
            return CEC_ERR_INVALID_ARGUMENT;
        }
    }
    int dev = 0;
    CEC_TRY(current_device(&dev));
    cec_codec* c = const_cast<cec_codec*>(cc);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (async && device_plan_covers(c->d, c->p, n, data_only)) {
        g_device_planned.fetch_add(1, std::memory_order_relaxed);
        return read_ragged_async(c, base, offs, lens, n, present, expected, verified, part_status,
                                 data_only, s, ret);
    }
    if (async) g_host_planned.fetch_add(1, std::memory_order_relaxed);
    return read_ragged(c, base, offs, lens, n, present, expected, verified, part_status, data_only,
                       s);
}

// Host staged (cec_parts_encode, cec_parts_read, cec_parts_verify): the parts packed into an
// arena's pinned staging in the cec_ragged_layout layout, moved up, worked on as above, results
// copied out.

}  // namespace

// Their arenas: one per call in flight (and per batch of cec_part_read calls, percall.cpp).
ArenaPool& cec::ragged_arenas() {
    static ArenaPool* pool = new ArenaPool();
    return *pool;
}

namespace {

// fn(k) for k < n on up to 8 threads: one per 16 MiB of `bytes` moved, so a call of a few small
// parts never starts one.
template <typename Fn>
void for_parts(size_t n, size_t bytes, Fn fn) {
    const size_t nt = std::min<size_t>({size_t(8), bytes / (size_t(16) << 20), n});
    if (nt <= 1) {
        for (size_t k = 0; k < n; ++k) fn(k);
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < n;) fn(k);
    };
    std::vector<std::thread> th;
    for (size_t i = 1; i < nt; ++i) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
}

}  // namespace

// The packing of a host-staged encode: data chunk j of part k (L_k bytes at
// dst + offs[k] + j * stride(L_k)) = bytes [j*L, (j+1)*L) of the caller's lengths[k] bytes, zeros
// behind.  Only those bytes are read.
// With seg_offs / seg_lens (the segment pipeline): piece j of entry k is the columns
// [seg_offs[k], + seg_lens[k]) of that chunk, seg_lens[k] bytes at dst + offs[k] + j *
// stride(seg_lens[k]).
void cec::pack_parts(uint8_t* dst, const size_t* offs, size_t d, const uint8_t* const* bufs,
                     const size_t* lengths, const size_t* chunk_lens, size_t n,
                     const size_t* seg_offs, const size_t* seg_lens) {
    size_t in_bytes = 0;
    for (size_t k = 0; k < n; ++k) in_bytes += seg_lens ? d * seg_lens[k] : lengths[k];
    for_parts(n, in_bytes, [&](size_t k) {
        const size_t L = chunk_lens[k], len = lengths[k];
        const size_t piece = seg_lens ? seg_lens[k] : L, cs = ragged_stride(piece);
        for (size_t j = 0; j < d; ++j) {
            uint8_t* to = dst + offs[k] + j * cs;
            const size_t b0 = j * L + (seg_offs ? seg_offs[k] : 0);
            const size_t have = b0 < len ? std::min(piece, len - b0) : 0;
            if (have) std::memcpy(to, bufs[k] + b0, have);
            if (have < piece) std::memset(to + have, 0, piece - have);
        }
    });
}

// The packing of a host-staged read: every loaded chunk (present[k * t + i] != 0) of part k, L_k
// bytes at shards[k * t + i], to dst + offs[k] + i * stride(L_k).  Only those are read.
void cec::pack_loaded(uint8_t* dst, const size_t* offs, size_t t, const uint8_t* const* shards,
                      const size_t* chunk_lens, size_t n, const uint8_t* present) {
    size_t in_bytes = 0;
    for (size_t k = 0; k < n; ++k)
        for (size_t i = 0; i < t; ++i) in_bytes += present[k * t + i] ? chunk_lens[k] : 0;
    for_parts(n, in_bytes, [&](size_t k) {
        const size_t L = chunk_lens[k], cs = ragged_stride(L);
        for (size_t i = 0; i < t; ++i)
            if (present[k * t + i]) std::memcpy(dst + offs[k] + i * cs, shards[k * t + i], L);
    });
}

// The packed split layout: part k+1 directly behind part k in each region.
int cec::split_layout(size_t d, size_t p, const size_t* lens, size_t n, size_t* doffs,
                      size_t* poffs, size_t* data_bytes, size_t* parity_bytes) {
    CEC_TRY(ragged_layout(d, lens, n, doffs, data_bytes));
    return ragged_layout(p, lens, n, poffs, parity_bytes);
}

// Copies of the byte ranges [first, second) (ascending, disjoint) between the staging and the
// device arena, which share their offsets.  Neighbouring ranges share one copy, with what lies
// between them travelling along, until the gap is worth a copy call of its own (256 KiB: a few
// microseconds of the link either way).
int cec::copy_spans(uint8_t* stage, uint8_t* dbase, const Spans& spans, bool to_device,
                    hipStream_t s) {
    constexpr size_t kGap = size_t(256) << 10;
    for (size_t q = 0; q < spans.size();) {
        const size_t from = spans[q].first;
        size_t to = spans[q].second;
        for (++q; q < spans.size() && spans[q].first - to < kGap; ++q) to = spans[q].second;
        if (to_device)
            HIP_TRY(hipMemcpyAsync(dbase + from, stage + from, to - from, hipMemcpyHostToDevice, s));
        else
            HIP_TRY(hipMemcpyAsync(stage + from, dbase + from, to - from, hipMemcpyDeviceToHost, s));
    }
    return CEC_OK;
}

// One round's place in an arena (Round, capi_internal.hpp).
int cec::reserve_round(Arena& a, size_t d, size_t t, const size_t* chunk_lens, size_t n, Round* r) {
    r->offs.resize(n);
    size_t total = 0;
    CEC_TRY(ragged_layout(t, chunk_lens, n, r->offs.data(), &total));
    const size_t cap = coalesce_max_bytes();
    CEC_TRY(a.in.reserve(total, cap / d * t + t * kRaggedAlign));
    CEC_TRY(a.out.reserve(n * t * 32, cap / 8));
    const size_t dig_bytes = round_up(n * t * 32, kChunkAlign);
    CEC_TRY(ctx_reserve(a.dev, dig_bytes + total));
    r->stage = a.in.ptr;
    r->dside = a.dev.dbuf;
    r->dbase = a.dev.dbuf + dig_bytes;
    r->s = a.dev.stream;
    return CEC_OK;
}

namespace {

// The rounds of a host-staged call over parts of d data chunks among t, of these chunk lengths:
// at most CEC_COALESCE_MAX_MIB of (padded) data chunks each, a larger part alone.  Every round is
// checked before the first one runs, so an error leaves the outputs untouched.  Then
// round(arena, k0, k1) for each, on one arena; nothing of a failed round stays in flight.
template <typename Fn>
int run_rounds(size_t d, size_t t, const size_t* chunk_lens, size_t n, Fn round) {
    const size_t cap = coalesce_max_bytes();
    std::vector<size_t> round_end;
    size_t bytes = 0, first = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t cs = ragged_stride(chunk_lens[k]);
        size_t b = 0;
        if (!cs || __builtin_mul_overflow(d, cs, &b)) return CEC_ERR_INVALID_ARGUMENT;
        if (k > first && (b > cap || bytes > cap - b)) {
            round_end.push_back(k);
            first = k;
            bytes = 0;
        }
        bytes += std::min(b, cap);
    }
    round_end.push_back(n);
    std::vector<size_t> offs(n);
    size_t k0 = 0, total = 0;
    for (size_t k1 : round_end) {
        CEC_TRY(ragged_layout(t, chunk_lens + k0, k1 - k0, offs.data(), &total));
        CEC_TRY(ragged_check(t, nullptr, offs.data(), chunk_lens + k0, k1 - k0));
        k0 = k1;
    }
    int dev = 0;
    CEC_TRY(current_device(&dev));
    Arena* arena = ragged_arenas().take(dev);
    int st = CEC_OK;
    k0 = 0;
    for (size_t k1 : round_end) {
        st = round(*arena, k0, k1);
        if (st != CEC_OK) break;
        k0 = k1;
    }
    if (st != CEC_OK && arena->dev.stream) {
        (void)hipStreamSynchronize(arena->dev.stream);
        (void)hipGetLastError();
    }
    ragged_arenas().give(dev, arena);
    return st;
}

// One round of cec_parts_encode: parts [0, n) of these arrays, packed, moved, encoded and hashed
// together, results copied out.
int parts_round(cec_codec* c, Arena& a, const uint8_t* const* bufs, const size_t* lengths,
                size_t n, uint8_t* const* parity_outs, uint8_t* digests_out,
                const size_t* chunk_lens) {
    const size_t d = c->d, p = c->p, t = d + p;
    Round r;
    CEC_TRY(reserve_round(a, d, t, chunk_lens, n, &r));
    const std::vector<size_t>& offs = r.offs;
    size_t out_bytes = 0;
    Spans parity;  // per part, behind its data chunks
    for (size_t k = 0; k < n; ++k) {
        const size_t cs = ragged_stride(chunk_lens[k]);
        out_bytes += p * chunk_lens[k];
        parity.emplace_back(offs[k] + d * cs, offs[k] + t * cs);
    }
    pack_parts(r.stage, offs.data(), d, bufs, lengths, chunk_lens, n);
    HIP_TRY(hipMemcpyAsync(r.dbase, r.stage, parity.back().first, hipMemcpyHostToDevice, r.s));
    CEC_TRY(ragged_launch(c, r.dbase, offs.data(), r.dbase, nullptr, chunk_lens, n, r.dside, r.s));
    // The parity comes back into the staging at its own offsets; the data chunks between two
    // parts' parity travel along while they are short (copy_spans).
    CEC_TRY(copy_spans(r.stage, r.dbase, parity, false, r.s));
    HIP_TRY(hipMemcpyAsync(a.out.ptr, r.dside, n * t * 32, hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipStreamSynchronize(r.s));
    for_parts(n, out_bytes, [&](size_t k) {
        const size_t L = chunk_lens[k];
        for (size_t i = 0; i < p; ++i)
            std::memcpy(parity_outs[k] + i * L, r.stage + parity[k].first + i * ragged_stride(L), L);
    });
    std::memcpy(digests_out, a.out.ptr, n * t * 32);
    return CEC_OK;
}

}  // namespace

// The steps of one round of a host-staged read (capi_internal.hpp).  The loaded chunks are packed
// into the arena and moved up, verified and rebuilt as in cec_read_ragged, and only the rebuilt
// chunks come back, into the caller's slots.
void cec::read_round_stage(const Round& r, size_t k, size_t t, size_t L, uint8_t* const* shards,
                           const uint8_t* present) {
    const size_t cs = ragged_stride(L);
    for (size_t i = 0; i < t; ++i)
        if (present[i]) std::memcpy(r.stage + r.offs[k] + i * cs, shards[i], L);
}

int cec::read_round_launch(cec_codec* c, Arena& a, const Round& r, const size_t* chunk_lens,
                           size_t n, const uint8_t* present, bool data_only, uint8_t* verified,
                           int* part_status) {
    const size_t d = c->d, t = c->d + c->p, items = n * t;
    Spans spans;
    plan::loaded_spans(t, chunk_lens, r.offs.data(), n, present, &spans);
    HIP_TRY(hipMemcpyAsync(r.dside, a.out.ptr, items * 32, hipMemcpyHostToDevice, r.s));
    CEC_TRY(copy_spans(r.stage, r.dbase, spans, true, r.s));
    CEC_TRY(read_ragged(c, r.dbase, r.offs.data(), chunk_lens, n, present, r.dside, verified,
                        part_status, data_only, r.s));
    // what the rebuild wrote: in a decodable part, every slot of the mode that did not verify
    spans.clear();
    plan::rebuilt_spans(d, t, chunk_lens, r.offs.data(), n, verified, part_status, data_only,
                        &spans);
    CEC_TRY(copy_spans(r.stage, r.dbase, spans, false, r.s));
    HIP_TRY(hipStreamSynchronize(r.s));
    return CEC_OK;
}

void cec::read_round_collect(const Round& r, size_t k, size_t d, size_t t, size_t L,
                             uint8_t* const* shards, const uint8_t* verified, int part_status,
                             bool data_only) {
    const size_t cs = ragged_stride(L);
    for (size_t i = 0; i < t; ++i)
        if (plan::rebuilt_slot(i, d, data_only, verified[i], part_status))
            std::memcpy(shards[i], r.stage + r.offs[k] + i * cs, L);
}

namespace {

// One round of cec_parts_read: parts [0, n) of these arrays, through the steps above.
int parts_read_round(cec_codec* c, Arena& a, uint8_t* const* shards, const size_t* chunk_lens,
                     size_t n, const uint8_t* present, const uint8_t* expected, bool data_only,
                     uint8_t* verified, int* part_status) {
    const size_t d = c->d, t = c->d + c->p, items = n * t;
    Round r;
    CEC_TRY(reserve_round(a, d, t, chunk_lens, n, &r));
    size_t out_bytes = 0;
    pack_loaded(r.stage, r.offs.data(), t, shards, chunk_lens, n, present);
    std::memcpy(a.out.ptr, expected, items * 32);
    CEC_TRY(read_round_launch(c, a, r, chunk_lens, n, present, data_only, verified, part_status));
    for (size_t k = 0; k < n; ++k)
        for (size_t i = 0; i < t; ++i)
            if (plan::rebuilt_slot(i, d, data_only, verified[k * t + i], part_status[k]))
                out_bytes += chunk_lens[k];
    for_parts(n, out_bytes, [&](size_t k) {
        read_round_collect(r, k, d, t, chunk_lens[k], shards + k * t, verified + k * t,
                           part_status[k], data_only);
    });
    return CEC_OK;
}

// One round of cec_parts_verify: copies [0, n) of these arrays, a ragged layout of one chunk per
// part.  The copies are packed into the arena and moved up in one copy (the padding between them,
// under 16 bytes each, travels along), verified as in cec_verify_ragged, and only the flags come
// back.
int parts_verify_round(Arena& a, const uint8_t* const* bufs, const size_t* lens, size_t n,
                       const uint8_t* expected, uint8_t* ok) {
    Round r;
    CEC_TRY(reserve_round(a, 1, 1, lens, n, &r));
    size_t in_bytes = 0;
    for (size_t k = 0; k < n; ++k) in_bytes += lens[k];
    for_parts(n, in_bytes, [&](size_t k) { std::memcpy(r.stage + r.offs[k], bufs[k], lens[k]); });
    std::memcpy(a.out.ptr, expected, n * 32);
    HIP_TRY(hipMemcpyAsync(r.dside, a.out.ptr, n * 32, hipMemcpyHostToDevice, r.s));
    HIP_TRY(hipMemcpyAsync(r.dbase, r.stage, r.offs[n - 1] + lens[n - 1], hipMemcpyHostToDevice,
                           r.s));
    return verify_ragged(r.dbase, r.offs.data(), lens, n, 1, nullptr, r.dside, ok, r.s);
}

}  // namespace

extern "C" {

size_t cec_ragged_stride(size_t chunk_len) { return ragged_stride(chunk_len); }

void cec_ragged_stats(uint64_t* fused, uint64_t* two_pass) {
    if (fused) *fused = g_fused_seqs.load();
    if (two_pass) *two_pass = g_two_pass_seqs.load();
}

int cec_ragged_layout(size_t total_shards, const size_t* chunk_lens, size_t n_parts,
                      size_t* part_offsets, size_t* total_bytes) {
    if (!total_bytes || total_shards == 0) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts && (!chunk_lens || !part_offsets)) return CEC_ERR_INVALID_ARGUMENT;
    return ragged_layout(total_shards, chunk_lens, n_parts, part_offsets, total_bytes);
}

int cec_encode_hash_ragged(const cec_codec* cc, uint8_t* base, const size_t* part_offsets,
                           const size_t* chunk_lens, size_t n_parts, uint8_t* digests,
                           void* stream) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!base || !part_offsets || !chunk_lens || !digests) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(ragged_check(cc->d + cc->p, base, part_offsets, chunk_lens, n_parts));
    return ragged_launch(const_cast<cec_codec*>(cc), base, part_offsets, base, nullptr, chunk_lens,
                         n_parts, digests, static_cast<hipStream_t>(stream));
}

int cec_split_layout(size_t data_shards, size_t parity_shards, const size_t* chunk_lens,
                     size_t n_parts, size_t* data_offsets, size_t* parity_offsets,
                     size_t* data_bytes, size_t* parity_bytes) {
    if (!data_bytes || !parity_bytes || data_shards == 0 || parity_shards == 0)
        return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts && (!chunk_lens || !data_offsets || !parity_offsets))
        return CEC_ERR_INVALID_ARGUMENT;
    return split_layout(data_shards, parity_shards, chunk_lens, n_parts, data_offsets,
                        parity_offsets, data_bytes, parity_bytes);
}

int cec_encode_hash_split(const cec_codec* cc, const uint8_t* data_base,
                          const size_t* data_offsets, uint8_t* parity_base,
                          const size_t* parity_offsets, const size_t* chunk_lens, size_t n_parts,
                          uint8_t* digests, void* stream) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!data_base || !data_offsets || !parity_base || !parity_offsets || !chunk_lens || !digests)
        return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(split_check(cc->d, cc->p, data_base, data_offsets, parity_base, parity_offsets,
                        chunk_lens, n_parts));
    return ragged_launch(const_cast<cec_codec*>(cc), data_base, data_offsets, parity_base,
                         parity_offsets, chunk_lens, n_parts, digests,
                         static_cast<hipStream_t>(stream));
}

size_t cec_sha_midstate_bytes(void) { return plan::kMidstateBytes; }

int cec_encode_hash_segments(const cec_codec* cc, const uint8_t* data_base,
                             const size_t* data_offsets, uint8_t* parity_base,
                             const size_t* parity_offsets, const size_t* seg_lens, size_t n_segs,
                             const uint32_t* state_slots, const uint8_t* flags, uint8_t* midstates,
                             size_t n_state_slots, uint8_t* digests, void* stream) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n_segs == 0) return CEC_OK;
    if (!data_base || !data_offsets || !parity_base || !parity_offsets || !seg_lens ||
        !state_slots || !flags || !digests)
        return CEC_ERR_INVALID_ARGUMENT;
    size_t items = 0;  // SHA-256 items are 32-bit (checked before the arrays are walked)
    if (__builtin_mul_overflow(n_segs, cc->d + cc->p, &items) || items > 0xFFFFFFFFull)
        return CEC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; !midstates && k < n_segs; ++k)
        if (plan::touches_record(flags[k])) return CEC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < n_segs; ++k)
        if (seg_lens[k] == 0) return CEC_EMPTY_SHARD;
    if (reinterpret_cast<uintptr_t>(midstates) % kRaggedAlign) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(segments_check(cc->d, cc->p, data_base, data_offsets, parity_base, parity_offsets,
                           seg_lens, n_segs, state_slots, flags, n_state_slots));
    int dev = 0;
    CEC_TRY(current_device(&dev));
    return segments_launch(const_cast<cec_codec*>(cc), data_base, data_offsets, parity_base,
                           parity_offsets, seg_lens, n_segs, state_slots, flags, midstates, digests,
                           static_cast<hipStream_t>(stream));
}

int cec_parts_encode(const cec_codec* cc, const uint8_t* const* data_bufs, const size_t* lengths,
                     size_t n_parts, uint8_t* const* parity_outs, uint8_t* digests_out,
                     size_t* chunksizes) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!data_bufs || !lengths || !parity_outs || !digests_out || !chunksizes)
        return CEC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < n_parts; ++k)
        if (lengths[k] == 0) return CEC_EMPTY_SHARD;
    for (size_t k = 0; k < n_parts; ++k)
        if (!data_bufs[k] || !parity_outs[k]) return CEC_ERR_INVALID_ARGUMENT;
    cec_codec* c = const_cast<cec_codec*>(cc);
    const size_t t = c->d + c->p;
    std::vector<size_t> L(n_parts);
    for (size_t k = 0; k < n_parts; ++k) L[k] = (lengths[k] - 1) / c->d + 1;
    CEC_TRY(run_rounds(c->d, t, L.data(), n_parts, [&](Arena& a, size_t k0, size_t k1) {
        return parts_round(c, a, data_bufs + k0, lengths + k0, k1 - k0, parity_outs + k0,
                           digests_out + k0 * t * 32, L.data() + k0);
    }));
    std::copy(L.begin(), L.end(), chunksizes);
    return CEC_OK;
}

int cec_reconstruct_ragged(const cec_codec* cc, uint8_t* base, const size_t* part_offsets,
                           const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                           int data_only, void* stream) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!base || !part_offsets || !chunk_lens || !present) return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(ragged_check(cc->d + cc->p, base, part_offsets, chunk_lens, n_parts));
    CEC_TRY(check_present(cc->d, cc->d + cc->p, present, n_parts));
    int dev = 0;
    CEC_TRY(current_device(&dev));
    return reconstruct_ragged(const_cast<cec_codec*>(cc), base, part_offsets, chunk_lens, n_parts,
                              present, data_only != 0, static_cast<hipStream_t>(stream));
}

int cec_verify_ragged(size_t total_shards, const uint8_t* base, const size_t* part_offsets,
                      const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                      const uint8_t* expected, uint8_t* verified, void* stream) {
    if (total_shards == 0) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!base || !part_offsets || !chunk_lens || !expected || !verified)
        return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(ragged_check(total_shards, base, part_offsets, chunk_lens, n_parts));
    int dev = 0;
    CEC_TRY(current_device(&dev));
    return verify_ragged(base, part_offsets, chunk_lens, n_parts, total_shards, present, expected,
                         verified, static_cast<hipStream_t>(stream));
}

int cec_verify_segments(const uint8_t* base, const size_t* offsets, const size_t* seg_lens,
                        size_t n_segs, const uint32_t* state_slots, const uint8_t* flags,
                        uint8_t* midstates, size_t n_state_slots, const uint8_t* expected,
                        uint8_t* ok, void* stream) {
    if (n_segs == 0) return CEC_OK;
    if (!base || !offsets || !seg_lens || !state_slots || !flags || !expected || !ok)
        return CEC_ERR_INVALID_ARGUMENT;
    // the kernel's item index is 32-bit (checked before the arrays are walked)
    if (n_segs > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;
    if (!midstates && !plan::all_whole(flags, n_segs)) return CEC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < n_segs; ++k)
        if (seg_lens[k] == 0) return CEC_EMPTY_SHARD;
    if (reinterpret_cast<uintptr_t>(midstates) % kRaggedAlign ||
        reinterpret_cast<uintptr_t>(expected) % kRaggedAlign)
        return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(ragged_check(1, base, offsets, seg_lens, n_segs));
    static const char* const kRule[] = {
        "", "an entry that is not CEC_SEG_LAST has a length that is no multiple of 64",
        "a state slot is not below n_state_slots",
        "two entries of one call name the same state slot"};
    if (const int rule = plan::scrub_rules(seg_lens, state_slots, flags, n_segs, n_state_slots)) {
        set_last_error(std::string("cec_verify_segments: ") + kRule[rule]);
        return CEC_ERR_INVALID_ARGUMENT;
    }
    int dev = 0;
    CEC_TRY(current_device(&dev));
    return verify_segments_launch(base, offsets, seg_lens, n_segs, state_slots, flags, midstates,
                                  expected, ok, static_cast<hipStream_t>(stream));
}

int cec_read_ragged(const cec_codec* c, uint8_t* base, const size_t* part_offsets,
                    const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                    const uint8_t* expected, uint8_t* verified, int* part_status, void* stream) {
    return read_ragged_checked(c, base, part_offsets, chunk_lens, n_parts, present, expected,
                               verified, part_status, true, stream);
}

int cec_resilver_ragged(const cec_codec* c, uint8_t* base, const size_t* part_offsets,
                        const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                        const uint8_t* expected, uint8_t* verified, int* part_status,
                        void* stream) {
    return read_ragged_checked(c, base, part_offsets, chunk_lens, n_parts, present, expected,
                               verified, part_status, false, stream);
}

int cec_read_ragged_packed_async(const cec_codec* c, uint8_t* base, const size_t* part_offsets,
                                 const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                                 const uint8_t* expected, int data_only, uint8_t* verified,
                                 int* part_status, uint8_t* rebuilt, size_t rebuilt_cap,
                                 size_t* rebuilt_offsets, void* stream) {
    const PackedReturn ret{rebuilt, rebuilt_cap, rebuilt_offsets};
    return read_ragged_checked(c, base, part_offsets, chunk_lens, n_parts, present, expected,
                               verified, part_status, data_only != 0, stream, true, &ret);
}

int cec_read_ragged_async(const cec_codec* c, uint8_t* base, const size_t* part_offsets,
                          const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                          const uint8_t* expected, uint8_t* verified, int* part_status,
                          void* stream) {
    return read_ragged_checked(c, base, part_offsets, chunk_lens, n_parts, present, expected,
                               verified, part_status, true, stream, true);
}

int cec_resilver_ragged_async(const cec_codec* c, uint8_t* base, const size_t* part_offsets,
                              const size_t* chunk_lens, size_t n_parts, const uint8_t* present,
                              const uint8_t* expected, uint8_t* verified, int* part_status,
                              void* stream) {
    return read_ragged_checked(c, base, part_offsets, chunk_lens, n_parts, present, expected,
                               verified, part_status, false, stream, true);
}

void cec_ragged_read_stats(uint64_t* device_planned, uint64_t* host_planned) {
    if (device_planned) *device_planned = g_device_planned.load();
    if (host_planned) *host_planned = g_host_planned.load();
}

int cec_parts_read(const cec_codec* cc, uint8_t* const* shards, const size_t* chunk_lens,
                   size_t n_parts, const uint8_t* present, const uint8_t* expected, int data_only,
                   uint8_t* verified, int* part_status) {
    if (!cc) return CEC_ERR_INVALID_ARGUMENT;
    if (n_parts == 0) return CEC_OK;
    if (!shards || !chunk_lens || !present || !expected || !verified || !part_status)
        return CEC_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < n_parts; ++k)
        if (chunk_lens[k] == 0) return CEC_EMPTY_SHARD;
    cec_codec* c = const_cast<cec_codec*>(cc);
    const size_t d = c->d, t = c->d + c->p;
    size_t items = 0;
    if (__builtin_mul_overflow(n_parts, t, &items) || items > 0xFFFFFFFFull)
        return CEC_ERR_INVALID_ARGUMENT;
    CEC_TRY(null_slot_rule("cec_parts_read", shards, present, n_parts, d, t, data_only != 0));
    return run_rounds(d, t, chunk_lens, n_parts, [&](Arena& a, size_t k0, size_t k1) {
        return parts_read_round(c, a, shards + k0 * t, chunk_lens + k0, k1 - k0, present + k0 * t,
                                expected + k0 * t * 32, data_only != 0, verified + k0 * t,
                                part_status + k0);
    });
}

int cec_parts_verify(const uint8_t* const* bufs, const size_t* lens, size_t n,
                     const uint8_t* expected, uint8_t* ok) {
    if (n == 0) return CEC_OK;
    if (!bufs || !lens || !expected || !ok) return CEC_ERR_INVALID_ARGUMENT;
    if (n > 0xFFFFFFFFull) return CEC_ERR_INVALID_ARGUMENT;  // before the arrays are walked
    for (size_t i = 0; i < n; ++i)
        if (lens[i] == 0) return CEC_EMPTY_SHARD;
    for (size_t i = 0; i < n; ++i)
        if (!bufs[i]) {
            set_last_error("cec_parts_verify: a copy is NULL");
            return CEC_ERR_INVALID_ARGUMENT;
        }
    return run_rounds(1, 1, lens, n, [&](Arena& a, size_t k0, size_t k1) {
        return parts_verify_round(a, bufs + k0, lens + k0, k1 - k0, expected + k0 * 32, ok + k0);
    });
}

}  // extern "C"
