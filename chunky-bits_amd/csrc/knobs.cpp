// Environment knobs, parsed once into an immutable snapshot (knobs.hpp).
#include "knobs.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>

#include "chunky_ec.h"

namespace cec {

namespace {

// "0" -> false, anything else set -> true, unset -> dflt
bool flag(const char* name, bool dflt) {
    const char* e = std::getenv(name);
    return e ? !(e[0] == '0') : dflt;
}

unsigned long long number(const char* name, unsigned long long dflt) {
    const char* e = std::getenv(name);
    return e ? std::strtoull(e, nullptr, 10) : dflt;
}

Knobs* parse() {
    auto* k = new Knobs();
    // Product knobs: capacities and diagnostics, and the test knobs that force one of the
    // product's own paths at test sizes (both arms are product code, picked by shape or size).
    k->apply_bs = flag("CEC_APPLY_BS", true);
    k->apply_max_blocks = number("CEC_APPLY_MAX_BLOCKS", 0);
    if (const char* e = std::getenv("CEC_SHA_VARIANT")) k->sha_variant = std::atoi(e);
    if (const char* e = std::getenv("CEC_FUSED_MODE")) k->fused_mode = std::atoi(e);
    if (const char* e = std::getenv("CEC_FUSED"))
        k->fused = e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1;
    if (const char* e = std::getenv("CEC_RAGGED_FUSED"))  // "0" or "1"; anything else: unset
        k->ragged_fused = (e[0] == '0' || e[0] == '1') && e[1] == '\0' ? e[0] - '0' : -1;
    if (const char* e = std::getenv("CEC_COALESCE_MIXED"))  // "0" or "1"; anything else: unset
        k->coalesce_mixed = (e[0] == '0' || e[0] == '1') && e[1] == '\0' ? e[0] - '0' : -1;
    k->coalesce_us = uint32_t(number("CEC_COALESCE_US", 200));
    k->coalesce_max_bytes = std::max<size_t>(size_t(number("CEC_COALESCE_MAX_MIB", 1024)), 1)
                            << 20;
    k->coalesce_trace = std::getenv("CEC_COALESCE_TRACE") != nullptr;
    k->coalesce_inflight =
        uint32_t(std::min<unsigned long long>(std::max(number("CEC_COALESCE_INFLIGHT", 2), 1ull), 16ull));
    if (std::getenv("CEC_IDLE_STAGING_MIB"))
        k->idle_staging_bytes = size_t(number("CEC_IDLE_STAGING_MIB", 1024)) << 20;
    k->multi_copy_threads = unsigned(
        std::min<unsigned long long>(std::max(number("CEC_MULTI_COPY_THREADS", 4), 1ull), 32ull));
    return k;
}

std::atomic<const Knobs*> g_knobs{nullptr};
std::mutex g_parse_mu;

}  // namespace

const Knobs& knobs() {
    const Knobs* k = g_knobs.load(std::memory_order_acquire);
    if (k) return *k;
    std::lock_guard<std::mutex> lk(g_parse_mu);
    k = g_knobs.load(std::memory_order_acquire);
    if (!k) {
        k = parse();
        g_knobs.store(k, std::memory_order_release);
    }
    return *k;
}

void reload_knobs() {
    std::lock_guard<std::mutex> lk(g_parse_mu);
    // the old snapshot stays allocated: a launch on another thread may still be reading it
    g_knobs.store(parse(), std::memory_order_release);
}

}  // namespace cec

extern "C" void cec_reload_knobs(void) { cec::reload_knobs(); }
