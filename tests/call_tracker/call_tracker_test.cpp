// CPU driver for mm::CallTracker (mirror-maze_amd/csrc/mm_calls.cpp): a tracker of 4 status slots that keeps 2
// failed calls, over an array of words this program writes itself, as the device would.
// Usage: call_tracker_test <case>; prints "ok <case>" and exits 0, or the first failed check and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mm_api.h"
#include "mm_calls.h"

using namespace mm;

namespace {

constexpr uint32_t kSlots = 4;
constexpr size_t kKept = 2;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                       \
        }                                                                  \
    } while (0)
#define CHECK_EQ(a, b)                                                                      \
    do {                                                                                    \
        const auto va = (a);                                                                \
        const auto vb = (b);                                                                \
        if (!(va == vb)) {                                                                  \
            printf("FAILED %s:%d: %s == %s\n  got:  %s\n  want: %s\n", __FILE__, __LINE__, #a, #b, \
                   show(va).c_str(), show(vb).c_str());                                     \
            exit(1);                                                                        \
        }                                                                                   \
    } while (0)
std::string show(const std::string& s) { return s; }
std::string show(const char* s) { return s; }
std::string show(unsigned long long v) { return std::to_string(v); }
std::string show(int v) { return std::to_string(v); }
std::string show(unsigned v) { return std::to_string(v); }
std::string show(unsigned long v) { return std::to_string(v); }
std::string show(const std::vector<int>& v) {
    std::string s = "[";
    for (int x : v) s += std::to_string(x) + " ";
    return s + "]";
}

// The words, the tracker over them and what its wait callback saw.
struct Rig {
    uint32_t words[kSlots + kRingDiagWords];
    std::vector<int> waits;
    int set_done_at = -1;  // the wait level at which the "device" finishes the awaited slot's launch
    uint32_t awaited = 0;
    int wait_rc = 0;
    std::string err;
    CallTracker t;

    explicit Rig(uint64_t first_launch = 0) {
        memset(words, 0xAB, sizeof(words));  // the tracker zeroes them
        t = CallTracker(words, [this](int level) {
            waits.push_back(level);
            if (level == set_done_at) finish(awaited, 0);
            return wait_rc;
        }, kSlots, kKept, first_launch);
    }
    // the device ends the launch in `slot`
    void finish(uint32_t slot, uint32_t bits) { __atomic_store_n(words + slot, bits | kStatusDone, __ATOMIC_RELEASE); }
    uint32_t launch() {
        uint32_t slot = 99;
        CHECK_EQ(t.next_status(slot, err), (int)MM_OK);
        CHECK(slot < kSlots);
        CHECK_EQ(words[slot], 0u);
        return slot;
    }
    // a call of one launch that ends with `bits`
    uint64_t call(const char* what, uint32_t bits) {
        const uint64_t id = t.begin_call();
        const uint32_t s = launch();
        t.end_call(what);
        finish(s, bits);
        return id;
    }
    void diag(uint32_t state, uint32_t launch_id) {
        uint32_t* d = words + kSlots;
        const uint32_t w[kRingDiagWords] = {state, 1, 1030, 3, 4, 5, 6, 7, 8, 9, 0, 0, 0x0000000Cu, 0x0000000Du, 14,
                                            launch_id};
        for (uint32_t i = 0; i < kRingDiagWords; ++i) d[i] = w[i];
    }
};

const char* const kNotEnqueued = "; this call was not enqueued";
const std::string kRingText = "tail ring wait timed out (kernel protocol error)";
std::string diag_text(uint32_t launch_id) {
    return " [first timed-out wait (launch " + std::to_string(launch_id) +
           "): reader of entry 1030 (slot 6, lap 2) in block 7 wave 8 lane 9 wanted turn 3, saw 4; reserved 5, "
           "claimed 6; gave up after 14 polls at device clock 55834574860]";
}

void clean_call() {
    Rig r;
    for (uint32_t i = 0; i < kSlots + kRingDiagWords; ++i) CHECK_EQ(r.words[i], 0u);
    CHECK_EQ(r.t.last_call(), 0ull);
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_ERR_INVALID);
    CHECK_EQ(r.err, "mm_call_status: no such call");
    CHECK_EQ(r.t.begin_call(), 1ull);
    const uint32_t s = r.launch();
    CHECK_EQ(s, 0u);
    CHECK_EQ(r.t.last_launch(), 0ull);
    r.t.end_call("a clean call");
    CHECK_EQ(r.t.last_call(), 1ull);
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_PENDING);
    CHECK_EQ(r.t.report_failure("", r.err), (int)MM_OK);
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_PENDING);
    r.finish(s, 0);
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_OK);
    CHECK_EQ(r.t.report_failure("", r.err), (int)MM_OK);
    CHECK_EQ(r.t.call_status(2, r.err), (int)MM_ERR_INVALID);
    CHECK(r.waits.empty());
}

void failing_launch() {
    Rig r;
    r.call("mm_trace_tile, frames 0..0, tile (0, 0) 8x8 / 1, 8 spp", kErrInjected);
    // the next enqueue: the runtime asks first, and returns what it gets without numbering a call
    CHECK_EQ(r.t.report_failure(kNotEnqueued, r.err), (int)MM_ERR_HIP);
    CHECK_EQ(r.err, "call #1 (mm_trace_tile, frames 0..0, tile (0, 0) 8x8 / 1, 8 spp) failed on the GPU: injected fault "
                    "(MM_OPT_FAULT_INJECT); this call was not enqueued");
    CHECK_EQ(r.t.last_call(), 1ull);
    // reported once
    CHECK_EQ(r.t.report_failure(kNotEnqueued, r.err), (int)MM_OK);
    // mm_call_status keeps naming it
    for (int i = 0; i < 2; ++i) {
        CHECK_EQ(r.t.call_status(1, r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #1 (mm_trace_tile, frames 0..0, tile (0, 0) 8x8 / 1, 8 spp) failed on the GPU: injected "
                        "fault (MM_OPT_FAULT_INJECT)");
    }
    // a failure first seen by mm_call_status is not reported again by the next call
    const uint64_t id2 = r.call("second", kErrStack);
    CHECK_EQ(id2, 2ull);
    CHECK_EQ(r.t.call_status(2, r.err), (int)MM_ERR_STACK);
    CHECK_EQ(r.err, "call #2 (second) failed on the GPU: traversal stack overflow (depth > 50)");
    CHECK_EQ(r.t.report_failure(kNotEnqueued, r.err), (int)MM_OK);
}

void multi_launch_call() {
    Rig r;
    CHECK_EQ(r.t.begin_call(), 1ull);
    const uint32_t s0 = r.launch();
    r.finish(s0, kErrStack);  // launch 0 fails ...
    for (int l = 1; l < 4; ++l) r.finish(r.launch(), 0);
    CHECK_EQ(r.launch(), s0);  // ... and launch 4 takes its slot while the call is still open
    CHECK(r.waits.empty());
    r.t.end_call("five launches");
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_PENDING);
    CHECK_EQ(r.t.report_failure("", r.err), (int)MM_OK);
    r.finish(s0, 0);
    CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_STACK);
    CHECK_EQ(r.err, "call #1 (five launches) failed on the GPU: traversal stack overflow (depth > 50)");
    // the same with the failed launch's slot reused by the NEXT call's launch, the first still pending
    Rig q;
    q.t.begin_call();
    const uint32_t a = q.launch();
    q.finish(a, kErrInjected);
    for (int l = 1; l < 4; ++l) q.launch();  // (not finished: the call stays pending)
    q.t.end_call("four launches");
    q.t.begin_call();
    CHECK_EQ(q.launch(), a);
    q.t.end_call("next");
    for (uint32_t s = 0; s < kSlots; ++s) q.finish(s, 0);
    CHECK_EQ(q.t.call_status(1, q.err), (int)MM_ERR_HIP);
    CHECK_EQ(q.err, "call #1 (four launches) failed on the GPU: injected fault (MM_OPT_FAULT_INJECT)");
    CHECK_EQ(q.t.call_status(2, q.err), (int)MM_OK);
}

// fills the four slots with launches that have not ended
void fill(Rig& r) {
    r.t.begin_call();
    for (uint32_t l = 0; l < kSlots; ++l) CHECK_EQ(r.launch(), l);
    r.t.end_call("fill");
    r.t.begin_call();
}

void occupant_not_done() {
    uint32_t slot = 99;
    {  // done after the stream wait
        Rig r;
        fill(r);
        r.set_done_at = 0;
        CHECK_EQ(r.t.next_status(slot, r.err), (int)MM_OK);
        CHECK_EQ(slot, 0u);
        CHECK_EQ(r.waits, (std::vector<int>{0}));
        CHECK_EQ(r.words[0], 0u);
    }
    {  // done only after the device wait
        Rig r;
        fill(r);
        r.set_done_at = 1;
        CHECK_EQ(r.t.next_status(slot, r.err), (int)MM_OK);
        CHECK_EQ(r.waits, (std::vector<int>{0, 1}));
        CHECK_EQ(r.t.last_launch(), 4ull);
    }
    {  // never done
        Rig r;
        fill(r);
        CHECK_EQ(r.t.next_status(slot, r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "status word of an earlier launch never completed");
        CHECK_EQ(r.waits, (std::vector<int>{0, 1}));
        CHECK_EQ(r.t.last_launch(), 3ull);  // no launch was numbered
    }
    {  // the wait itself fails: its code is passed on
        Rig r;
        fill(r);
        r.wait_rc = MM_ERR_HIP;
        r.err = "the callback's text";
        CHECK_EQ(r.t.next_status(slot, r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "the callback's text");
        CHECK_EQ(r.waits, (std::vector<int>{0}));
    }
    {  // an occupant that is done is not waited for
        Rig r;
        fill(r);
        r.finish(0, 0);
        CHECK_EQ(r.t.next_status(slot, r.err), (int)MM_OK);
        CHECK(r.waits.empty());
    }
}

void never_enqueued() {
    Rig r;
    r.t.begin_call();
    const uint32_t s = r.launch();
    r.t.release_unqueued();  // the enqueue failed: nothing will write the slot
    CHECK_EQ(r.words[s], kStatusDone);
    r.t.end_call("failed to enqueue");
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_OK);
    for (int l = 0; l < 12; ++l) {  // three laps over the slots
        CHECK_EQ(r.t.report_failure(kNotEnqueued, r.err), (int)MM_OK);
        const uint64_t id = r.call("lap", 0);
        CHECK_EQ(r.t.call_status(id, r.err), (int)MM_OK);
    }
    CHECK(r.waits.empty());
    CHECK_EQ(r.t.last_call(), 13ull);
    CHECK_EQ(r.t.last_launch(), 12ull);
}

void failed_list_overflow() {
    Rig r;
    r.call("clean", 0);
    r.call("first", kErrInjected);
    r.call("second", kErrInjected);
    r.call("third", kErrStack);
    CHECK_EQ(r.t.call_status(2, r.err), (int)MM_ERR_INVALID);
    CHECK_EQ(r.err, "mm_call_status: status of call #2 no longer kept (older than the last 2 failed calls)");
    CHECK_EQ(r.t.call_status(1, r.err), (int)MM_ERR_INVALID);  // clean, but that is no longer known
    CHECK_EQ(r.err, "mm_call_status: status of call #1 no longer kept (older than the last 2 failed calls)");
    CHECK_EQ(r.t.call_status(4, r.err), (int)MM_ERR_STACK);
    CHECK_EQ(r.err, "call #4 (third) failed on the GPU: traversal stack overflow (depth > 50)");
    CHECK_EQ(r.t.call_status(3, r.err), (int)MM_ERR_HIP);
    // the oldest kept failure not yet reported goes to the next call; there is none left
    CHECK_EQ(r.t.report_failure(kNotEnqueued, r.err), (int)MM_OK);
    const uint64_t id = r.call("later", 0);
    CHECK_EQ(r.t.call_status(id, r.err), (int)MM_OK);
}

void ring_record() {
    {  // belongs to the reported call: appended and consumed
        Rig r;
        r.diag(1, 0);
        r.call("rings", kErrRing);
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #1 (rings) failed on the GPU: " + kRingText + diag_text(0));
        CHECK_EQ(r.words[kSlots], 0u);
    }
    {  // of an older launch: freed, no text
        Rig r(10);
        r.diag(1, 5);
        r.call("rings", kErrRing);
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #1 (rings) failed on the GPU: " + kRingText);
        CHECK_EQ(r.words[kSlots], 0u);
    }
    {  // of a newer launch: left for its own call
        Rig r(10);
        r.diag(1, 11);
        r.call("rings", kErrRing);
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #1 (rings) failed on the GPU: " + kRingText);
        CHECK_EQ(r.words[kSlots], 1u);
        r.call("rings again", kErrRing);  // launch 11
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #2 (rings again) failed on the GPU: " + kRingText + diag_text(11));
        CHECK_EQ(r.words[kSlots], 0u);
    }
    {  // still being written: ignored
        Rig r;
        r.diag(2, 0);
        r.call("rings", kErrRing);
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #1 (rings) failed on the GPU: " + kRingText);
        CHECK_EQ(r.words[kSlots], 2u);
    }
    {  // launch numbers straddling 2^32: the record's id is the launch number's low 32 bits
        Rig r((1ull << 32) - 2);
        r.t.begin_call();
        uint32_t s[4];
        for (int l = 0; l < 4; ++l) s[l] = r.launch();  // launches 2^32 - 2 .. 2^32 + 1
        CHECK_EQ(r.t.last_launch(), (1ull << 32) + 1);
        r.t.end_call("across the wrap");
        r.diag(1, 1);  // written by launch 2^32 + 1
        for (int l = 0; l < 4; ++l) r.finish(s[l], l == 3 ? kErrRing : 0u);
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #1 (across the wrap) failed on the GPU: " + kRingText + diag_text(1));
        CHECK_EQ(r.words[kSlots], 0u);
        // a record from before the wrap is older than a call after it, one from after it newer than one before
        r.diag(1, 0xFFFFFFFFu);
        r.call("after the wrap", kErrRing);  // launch 2^32 + 2
        CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
        CHECK_EQ(r.err, "call #2 (after the wrap) failed on the GPU: " + kRingText);
        CHECK_EQ(r.words[kSlots], 0u);
        Rig q((1ull << 32) - 1);
        q.diag(1, 0);
        q.call("before the wrap", kErrRing);  // launch 2^32 - 1
        CHECK_EQ(q.t.report_failure("", q.err), (int)MM_ERR_HIP);
        CHECK_EQ(q.err, "call #1 (before the wrap) failed on the GPU: " + kRingText);
        CHECK_EQ(q.words[kSlots], 1u);
    }
}

void error_bits() {
    Rig r;
    const struct { uint32_t bit; const char* text; int code; } bits[] = {
        {kErrStack, "traversal stack overflow (depth > 50)", MM_ERR_STACK},
        {kErrRing, "tail ring wait timed out (kernel protocol error)", MM_ERR_HIP},
        {kErrInjected, "injected fault (MM_OPT_FAULT_INJECT)", MM_ERR_HIP},
        {kErrLost, "injected lost tail-ring entry (MM_OPT_FAULT_INJECT 4)", MM_ERR_HIP},
        {kErrPublish, "the launch's status could not be published (its error flag was read after a sync)", MM_ERR_HIP},
    };
    for (const auto& b : bits) {
        CHECK_EQ(r.t.error_text(b.bit, 0, 1), b.text);
        CHECK_EQ(CallTracker::error_code(b.bit), b.code);
        if (b.bit != kErrStack) {
            CHECK_EQ(CallTracker::error_code(b.bit | kErrStack), (int)MM_ERR_HIP);
            CHECK_EQ(r.t.error_text(b.bit | kErrStack, 0, 1), std::string(bits[0].text) + "; " + b.text);
        }
    }
    CHECK_EQ(r.t.error_text(4u, 0, 1), "unknown error");  // a bit no text knows
    CHECK_EQ(CallTracker::error_code(4u), (int)MM_ERR_HIP);
    // a launch whose status could not be published: its flag, read after a sync, is folded into its own slot
    r.t.begin_call();
    const uint32_t s = r.launch();
    r.t.fold_unpublished(kErrStack);
    CHECK_EQ(r.words[s], kErrStack | kErrPublish | kStatusDone);
    r.t.end_call("unpublished");
    CHECK_EQ(r.t.report_failure("", r.err), (int)MM_ERR_HIP);
    CHECK_EQ(r.err, std::string("call #1 (unpublished) failed on the GPU: ") + bits[0].text + "; " + bits[4].text);
}

const struct { const char* name; void (*run)(); } kCases[] = {
    {"clean_call", clean_call},
    {"failing_launch", failing_launch},
    {"multi_launch_call", multi_launch_call},
    {"occupant_not_done", occupant_not_done},
    {"never_enqueued", never_enqueued},
    {"failed_list_overflow", failed_list_overflow},
    {"ring_record", ring_record},
    {"error_bits", error_bits},
};

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (const auto& k : kCases) printf("%s\n", k.name);
        return 0;
    }
    for (const auto& k : kCases)
        if (argc == 2 && !strcmp(argv[1], k.name)) {
            k.run();
            printf("ok %s\n", k.name);
            return 0;
        }
    printf("usage: call_tracker_test <case> | --list\n");
    return 2;
}
