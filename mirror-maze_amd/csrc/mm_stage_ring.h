// mm_stage_ring.h — the staging ring of a call's small host-side tables: a pinned host ring and its device
// mirror, both `cap` 32-bit words, filled from `next` on.  A call's table goes into fresh words of the host ring
// (consumed when the call returns) and from there to the mirror by a copy on the context's stream, ahead of the
// launch that reads it: a later call's table never lands on that of a launch still running, and nothing waits
// for the GPU -- except when the ring is full: then everything the device has queued is waited for once, and
// the ring grows (up to `wrap_cap` words, from where on it wraps instead).  mm_ctx (mm_ctx.h) holds one ring for
// camera records and one for list tables; mm_trace_calls.hip stage() carries the policy out.
//
// The policy is a pure function, and this header plain C++ (no HIP): a stand-alone host program tests it
// (tests/trace_args).  Requests are multiples of 16 words, so every span starts on a 64-byte line.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mm {

struct RingPlace {
    size_t at = 0;      // word offset the request lands at
    bool wait = false;  // the device is waited for first: words handed out earlier are taken again
    size_t grow = 0;    // the capacity to allocate anew before that (0: the ring stays)
};
// Where a request of n words lands in a ring of `cap` words filled up to `next`.
inline RingPlace ring_place(size_t cap, size_t next, size_t n, size_t min_cap, size_t wrap_cap) {
    if (next + n <= cap) return {next, false, 0};
    const bool grow = n > cap || cap < wrap_cap;
    return {0, true, grow ? std::max({min_cap, 2 * cap, n}) : 0};
}

struct StageRing {
    size_t min_cap, wrap_cap;  // words
    uint32_t* host = nullptr;
    uint32_t* dev = nullptr;
    size_t cap = 0, next = 0;
};

}  // namespace mm
