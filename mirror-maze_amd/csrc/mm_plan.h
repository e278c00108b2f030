// mm_plan.h — the launch policy of the trace calls as pure functions of scene
// facts, options and the tile: which query method, which LDS placement, tail
// deferral and its ring kind, fused resolve, rows per launch.  Plain C++ (no
// HIP): mm_trace_calls.hip gathers the inputs and carries the plan out.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "mm_api.h"
#include "mm_variants.h"

namespace mm {

// Staged samples (tail deferral / no fused resolve) per launch: whole rows up
// to this many paths (12 B each: 6 GiB).  A multi-frame launch over the cap
// runs without deferral (fused resolve) or is refused.
constexpr uint64_t kStagePathsMax = 1ull << 29;

// What mm_upload_scene found out about the scene.
struct SceneFacts {
    bool grid_ok = false;    // the certified grid search applies
    bool grid_slow = false;  // the grid has SLOW records (general rect test)
    bool grid_wide = false;  // 64-bit cell words with per-face list ranges
    bool grid_flat = false;  // the maze forms apply (grid_build.h GridHost::flat_ok)
    bool lean_ok = false;    // no SLOW rect records (loop form 7, grid search)
    uint32_t n_nodes = 0, n_rects = 0;  // production node array length, rects
    uint32_t bytes = 0, off_box = 0, off_data = 0;  // the grid image: its size and section offsets
    const char* grid_why = "";  // why there is no grid
};

// The options the policy reads (mm_ctx.h opt_*, include/mm_api.h MM_OPT_*).
struct PlanOptions {
    int pipe = MM_PIPE_AUTO;
    int opt_ww = -1;
    bool opt_lds = true;
    int opt_lds_rects = 1;
    bool opt_fuse = true;
    int opt_persist = 2;
    int opt_defer = -1;
    uint32_t opt_defer_min = 1u << 24;
    int opt_predraw = -1;
    bool opt_predraw_pool = true;
};

struct Choice {
    int form = 0, mode = 0;
    int code = MM_OK;  // else `error` is the text
    std::string error;
};
// The query method for the scene and MM_OPT_TRAVERSAL: a BVH loop form, or the grid form with its slow /
// wide / flat variants applied.  (The `mode` of the result is unused.)
Choice choose_method(const SceneFacts& f, const PlanOptions& o);
// The LDS placement of the wave-persistent kernel for choose_method's form; the form changes where the
// placement needs another (a grid whose index does not fit LDS: auto takes the BVH).
Choice choose_placement(const SceneFacts& f, const PlanOptions& o, int form);

// Bytes the placement stages (dynamic LDS, or the static grid array's content).
inline size_t lds_stage_bytes(const SceneFacts& f, int mode) {
    return lds_stage_bytes(mode, f.n_nodes, f.n_rects, f.bytes, f.off_data, f.off_box);
}

struct LaunchPlan {
    bool defer = false;  // mirror-tail deferral (the tail rings)
    int ring = 0;        // its ring kind: 1 records in global memory, 2 in LDS
    bool fuse = false;   // resolve fused into the trace kernel
    uint32_t rows_per_batch = 0;
    uint32_t predraw = 0;  // trials a new-path chunk pre-draws per path (wave-persistent kernel)
    uint32_t predraw_pool = 0;  // accepted trials the pooled rounds top a window up to (0: no pooled rounds)
    int code = MM_OK;    // else `error` is the text
    std::string error;
};
constexpr size_t kNotBuilt = ~(size_t)0;
// static_lds[k - 1]: the static LDS (sharedSizeBytes) of the deferral kernel with ring kind k, or kNotBuilt.
// multi_fn: null for a single-frame call, else the name of the multi-frame entry point the call came through.
// Trials a new-path chunk of the wave-persistent kernel draws into each path's window before its bounces
// (MM_OPT_PREDRAW; -1: by the bounce limit and by whether pooled rounds follow, MM_OPT_PREDRAW_POOL), and the
// accepted trials those pooled rounds top each window up to (0: none).
uint32_t plan_predraw(int opt_predraw, bool pool, uint32_t bounce_limit);
uint32_t plan_predraw_pool(bool pool, uint32_t bounce_limit);
LaunchPlan plan_tile(const SceneFacts& f, const PlanOptions& o, int form, int mode, const size_t static_lds[2],
                     const mm_ext& e, uint32_t w, uint32_t h, uint32_t n_frames, const char* multi_fn);

// A pixel-list launch (mm_trace_pixels): n_pixels entries of e.spp samples in ONE launch, w = n_pixels, h = 1.
// The list instances are the plain body's (no tail rings): never deferral, whatever MM_OPT_DEFER /
// MM_OPT_DEFER_MIN say (MM_PIPE_WAVEFRONT, deferral always on, is refused); the resolve is fused iff
// 64 % spp == 0 and MM_OPT_FUSE_RESOLVE, else the samples are staged.  MM_ERR_INVALID: the queue, n_pixels *
// spp in chunks padded to 64, beyond the 32-bit counter (less the 2^24 the waves' last claims may overshoot),
// or staged samples beyond kStagePathsMax.  rows_per_batch is 1.
LaunchPlan plan_pixels(const PlanOptions& o, const mm_ext& e, uint64_t n_pixels);
// A ray-list launch (mm_trace_rays): n_rays entries of e.spp samples in ONE launch, w = n_rays, h = 1, by
// plan_pixels' rule throughout -- no tail rings (MM_PIPE_WAVEFRONT: MM_ERR_UNSUPPORTED), the same fuse / stage
// choice, the same queue and staging bounds; the texts carry the call's name.
LaunchPlan plan_rays(const PlanOptions& o, const mm_ext& e, uint64_t n_rays);

// The pixel lists of several frames in ONE launch (mm_trace_pixel_lists): list f is entries offsets[f] ..
// offsets[f + 1] - 1 of the concatenated pixel array.  Each list's paths, entries * spp, are padded to whole
// 64-path chunks, so every list starts on a chunk boundary and a chunk belongs to one list.
struct ListSpan {
    uint32_t first_chunk = 0, n_chunks = 0;  // of the launch's queue
    uint32_t first_entry = 0, n_entries = 0;  // of the concatenation (offsets[f], offsets[f + 1] - offsets[f])
    uint32_t n_paths = 0;                     // n_entries * spp
};
struct ListsPlan {
    LaunchPlan plan;              // fuse-or-stage by plan_pixels' rule; code / error as there
    uint64_t n_entries = 0;       // offsets[n_lists]
    uint32_t n_chunks = 0;        // the queue, in chunks
    std::vector<ListSpan> lists;  // n_lists spans (an empty list: n_chunks 0, its successor's first_chunk)
};
// The entries of all lists, offsets[n_lists], or the refusal: a null `offsets`, n_lists outside 1..65535,
// offsets[0] != 0, or a decreasing offset (code MM_ERR_INVALID and the text in `error`).
int lists_total(const uint64_t* offsets, uint32_t n_lists, uint64_t& total, std::string& error);
// MM_ERR_INVALID: lists_total's refusals; the queue -- the sum of the lists' padded paths -- beyond the 32-bit
// counter (less the 2^24 the waves' last claims may overshoot); staged samples beyond kStagePathsMax.
// MM_ERR_UNSUPPORTED: MM_PIPE_WAVEFRONT.  A total of 0 entries is a valid plan with no chunks.
ListsPlan plan_pixel_lists(const PlanOptions& o, const mm_ext& e, const uint64_t* offsets, uint32_t n_lists);
// The list chunk `chunk` (< the queue's chunks) belongs to, by the search the kernel runs over the table of
// first chunks (first[0 .. n_lists], first[n_lists] = the queue's chunks): the last f with first[f] <= chunk.
inline uint32_t list_of_chunk(const uint32_t* first, uint32_t n_lists, uint32_t chunk) {
    uint32_t lo = 0, hi = n_lists;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace mm
