// mm_calls.h — mm::CallTracker: the per-launch status words of a context and
// the numbered calls that own them.  Plain C++ (no HIP): the runtime hands it
// the host-mapped words the kernels write, a test hands it an array and writes
// the words itself.
//
// Launch L of the context writes word L % slots when it ends (error bits |
// kStatusDone).  Each trace / query call is a numbered "call" owning a run of
// launches; a call whose launches raised an error is reported, naming the
// call, by the next call on the context, mm_sync or mm_call_status -- never
// blamed on a later call's work.
#pragma once

#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <string>
#include <vector>

namespace mm {

// Error flag bits (aux word 4, and the status word's low bits).
constexpr uint32_t kErrStack = 1u, kErrRing = 2u, kErrInjected = 8u, kErrLost = 16u, kErrPublish = 32u;
constexpr uint32_t kStatusDone = 0x80000000u;
// After the status words: the first timed-out ring wait's record (trace_kernels.hip ring_timeout).
constexpr uint32_t kRingDiagWords = 16;

class CallTracker {
public:
    // Waits for the device: level 0 the context's stream, level 1 the whole device.  Returns 0, or the
    // error code to pass on (the callback has recorded its own text).
    using Wait = std::function<int(int level)>;

    CallTracker() = default;
    // `words`: slots + kRingDiagWords words, zeroed here.
    CallTracker(uint32_t* words, Wait wait, uint32_t slots = 1024, size_t failed_kept = 64, uint64_t first_launch = 0);

    uint32_t slots() const { return slots_; }

    // ---- launches -----------------------------------------------------------
    // Takes the status slot of the next launch (`slot`: its word's index).  A slot still held by a launch
    // `slots` earlier that has not finished is waited for.
    int next_status(uint32_t& slot, std::string& err);
    uint64_t last_launch() const { return launch_seq_ - 1; }
    // The last launch was never enqueued: nothing will write its slot, which is released as finished-clean
    // (a slot left owned by a launch that never runs would fail every later call on the context).
    void release_unqueued();
    // The last launch ran but its status could not be published: `bits` is its error flag, read after a sync.
    void fold_unpublished(uint32_t bits);

    // ---- calls --------------------------------------------------------------
    uint64_t begin_call();                        // numbers a call; its launches are those taken from here on
    bool call_has_launches() const { return launch_seq_ > open_first_; }
    void end_call(const std::string& what);       // registers the call begun last, if it took a launch
    uint64_t last_call() const { return call_seq_; }

    void poll();  // folds finished calls' status words into the failed list (non-blocking)
    // The oldest unreported failed call, as the caller's return code (MM_OK: none).
    int report_failure(const char* suffix, std::string& err);
    // mm_call_status: MM_PENDING, MM_OK, or the call's error.
    int call_status(uint64_t call_id, std::string& err);

    // ---- texts --------------------------------------------------------------
    struct Failed { uint64_t id; uint32_t bits; std::string what; bool reported; };
    std::string ring_diag_text(uint64_t first, uint64_t n);
    std::string error_text(uint32_t bits, uint64_t first, uint64_t n);
    static int error_code(uint32_t bits);
    static std::string failed_text(const Failed& f);

private:
    struct Call { uint64_t id, first, n; std::string what; uint32_t bits; };
    uint32_t load(uint64_t launch) const { return __atomic_load_n(words_ + launch % slots_, __ATOMIC_ACQUIRE); }

    uint32_t* words_ = nullptr;
    Wait wait_;
    uint32_t slots_ = 0;
    size_t failed_kept_ = 0;
    std::vector<uint64_t> slot_owner_;  // launch id + 1 holding each slot, 0 = free
    uint64_t launch_seq_ = 0, call_seq_ = 0;
    uint64_t open_id_ = 0, open_first_ = 0;  // the call begun and not yet ended (0: none)
    uint32_t open_bits_ = 0;                 // error bits of its launches whose slots were reused already
    std::deque<Call> pending_;
    std::deque<Failed> failed_;    // the last failed_kept_ failed calls
    uint64_t failed_dropped_ = 0;  // highest call id dropped from failed_ (older ids: status no longer kept)
};

}  // namespace mm
