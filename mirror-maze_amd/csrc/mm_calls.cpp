// mm_calls.cpp — mm::CallTracker (mm_calls.h).
#include "mm_calls.h"

#include <algorithm>
#include <cstdio>
#include <utility>

#include "mm_api.h"
#include "mm_variants.h"

namespace mm {

namespace {
int fail(std::string& err, int code, const std::string& msg) {
    err = msg;
    return code;
}
}  // namespace

CallTracker::CallTracker(uint32_t* words, Wait wait, uint32_t slots, size_t failed_kept, uint64_t first_launch)
    : words_(words), wait_(std::move(wait)), slots_(slots), failed_kept_(failed_kept), slot_owner_(slots, 0),
      launch_seq_(first_launch), open_first_(first_launch) {
    std::fill(words_, words_ + slots_ + kRingDiagWords, 0u);
}

int CallTracker::next_status(uint32_t& slot, std::string& err) {
    const uint64_t id = launch_seq_;
    const uint32_t s = (uint32_t)(id % slots_);
    if (slot_owner_[s] && !(load(slot_owner_[s] - 1) & kStatusDone)) {
        if (int rc = wait_(0)) return rc;
        if (!(load(slot_owner_[s] - 1) & kStatusDone))
            if (int rc = wait_(1)) return rc;
        if (!(load(slot_owner_[s] - 1) & kStatusDone))
            return fail(err, MM_ERR_HIP, "status word of an earlier launch never completed");
    }
    if (slot_owner_[s]) {  // fold the finished occupant's bits into its call, if still pending
        const uint64_t prev = slot_owner_[s] - 1;
        for (auto& k : pending_)
            if (prev >= k.first && prev < k.first + k.n) k.bits |= load(prev) & ~kStatusDone;
        // the call still open (more launches than slots) is not in pending_ yet: end_call passes these on
        if (open_id_ && prev >= open_first_) open_bits_ |= load(prev) & ~kStatusDone;
    }
    __atomic_store_n(words_ + s, 0u, __ATOMIC_RELEASE);
    slot_owner_[s] = id + 1;
    launch_seq_ = id + 1;
    slot = s;
    return MM_OK;
}

void CallTracker::release_unqueued() {
    __atomic_store_n(words_ + last_launch() % slots_, kStatusDone, __ATOMIC_RELEASE);
}

void CallTracker::fold_unpublished(uint32_t bits) {
    // the kernel's error flag goes into THIS launch's slot, so it is never published by -- and
    // blamed on -- a later call's launch
    __atomic_store_n(words_ + last_launch() % slots_, bits | kErrPublish | kStatusDone, __ATOMIC_RELEASE);
}

uint64_t CallTracker::begin_call() {
    open_id_ = ++call_seq_;
    open_first_ = launch_seq_;
    open_bits_ = 0;
    return open_id_;
}

void CallTracker::end_call(const std::string& what) {
    if (call_has_launches()) pending_.push_back({open_id_, open_first_, launch_seq_ - open_first_, what, open_bits_});
    open_id_ = 0;
    open_first_ = launch_seq_;
    open_bits_ = 0;
}

// The record a timed-out ring wait left (trace_kernels.hip ring_timeout), as
// text, when it belongs to one of the launches [first, first + n) of the call
// being reported; consumed then (the device writes a new record only into a
// consumed one).  A record of an older launch than the call's is stale (its
// call was reported without it) and is dropped; a newer one is left for its
// own call.
std::string CallTracker::ring_diag_text(uint64_t first, uint64_t n) {
    uint32_t* d = words_ + slots_;
    if (__atomic_load_n(d, __ATOMIC_ACQUIRE) != 1u) return "";  // none, or being written (2)
    uint32_t w[kRingDiagWords];
    for (uint32_t i = 0; i < kRingDiagWords; ++i) w[i] = __atomic_load_n(d + i, __ATOMIC_RELAXED);
    const uint32_t rel = w[15] - (uint32_t)first;  // launch ids are the context's launch numbers, mod 2^32
    if (rel >= (uint32_t)n) {
        if ((int32_t)rel < 0) __atomic_store_n(d, 0u, __ATOMIC_RELEASE);  // stale: free the record
        return "";
    }
    const uint64_t t1 = w[12] | (uint64_t)w[13] << 32;
    char b[320];
    snprintf(b, sizeof(b),
             " [first timed-out wait (launch %u): %s of entry %u (slot %u, lap %u) in block %u wave %u lane %u "
             "wanted turn %u, saw %u; reserved %u, claimed %u; gave up after %u polls at device clock %llu]",
             w[15], w[1] == 1 ? "reader" : "writer", w[2], w[2] % kTailRing, w[2] / kTailRing, w[7], w[8], w[9],
             w[3], w[4], w[5], w[6], w[14], (unsigned long long)t1);
    __atomic_store_n(d, 0u, __ATOMIC_RELEASE);
    return b;
}

std::string CallTracker::error_text(uint32_t bits, uint64_t first, uint64_t n) {
    std::string s;
    auto add = [&](const std::string& m) { s += s.empty() ? m : std::string("; ") + m; };
    if (bits & kErrStack) add("traversal stack overflow (depth > 50)");
    if (bits & kErrRing) add("tail ring wait timed out (kernel protocol error)" + ring_diag_text(first, n));
    if (bits & kErrInjected) add("injected fault (MM_OPT_FAULT_INJECT)");
    if (bits & kErrLost) add("injected lost tail-ring entry (MM_OPT_FAULT_INJECT 4)");
    if (bits & kErrPublish) add("the launch's status could not be published (its error flag was read after a sync)");
    return s.empty() ? "unknown error" : s;
}

int CallTracker::error_code(uint32_t bits) { return (bits & ~kErrStack) ? MM_ERR_HIP : MM_ERR_STACK; }

void CallTracker::poll() {
    for (auto it = pending_.begin(); it != pending_.end();) {
        uint32_t bits = it->bits;
        bool done = true;
        for (uint64_t l = it->first; l < it->first + it->n && done; ++l) {
            // a slot reused by a later launch: this launch finished, its bits are in it->bits
            if (slot_owner_[l % slots_] != l + 1) continue;
            const uint32_t w = load(l);
            done = (w & kStatusDone) != 0;
            bits |= w & ~kStatusDone;
        }
        if (!done) { ++it; continue; }
        if (bits) {
            failed_.push_back({it->id, bits, it->what + " -- " + error_text(bits, it->first, it->n), false});
            if (failed_.size() > failed_kept_) {
                failed_dropped_ = std::max(failed_dropped_, failed_.front().id);
                failed_.pop_front();
            }
        }
        it = pending_.erase(it);
    }
}

// "call #N (what) failed on the GPU: why" (Failed::what holds "what -- why").
std::string CallTracker::failed_text(const Failed& f) {
    const size_t k = f.what.find(" -- ");
    return "call #" + std::to_string(f.id) + " (" + f.what.substr(0, k) + ") failed on the GPU: " +
           (k == std::string::npos ? std::string("unknown error") : f.what.substr(k + 4));
}

int CallTracker::report_failure(const char* suffix, std::string& err) {
    poll();
    for (auto& f : failed_)
        if (!f.reported) {
            f.reported = true;
            return fail(err, error_code(f.bits), failed_text(f) + suffix);
        }
    return MM_OK;
}

int CallTracker::call_status(uint64_t call_id, std::string& err) {
    if (call_id == 0 || call_id > call_seq_) return fail(err, MM_ERR_INVALID, "mm_call_status: no such call");
    poll();
    for (const auto& k : pending_)
        if (k.id == call_id) return MM_PENDING;
    for (auto& f : failed_)
        if (f.id == call_id) {
            f.reported = true;
            return fail(err, error_code(f.bits), failed_text(f));
        }
    // a finished call not in the failed list: clean -- unless failed calls as old as it were dropped from the list
    if (call_id <= failed_dropped_)
        return fail(err, MM_ERR_INVALID, "mm_call_status: status of call #" + std::to_string(call_id) +
                                             " no longer kept (older than the last " + std::to_string(failed_kept_) +
                                             " failed calls)");
    return MM_OK;
}

}  // namespace mm
