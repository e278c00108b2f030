// mm_plan.cpp — the launch policy (mm_plan.h).
#include "mm_plan.h"

#include <algorithm>

namespace mm {

namespace {
template <typename T>
T refuse(int code, const std::string& msg) {
    T r;
    r.code = code;
    r.error = msg;
    return r;
}
}  // namespace

// Auto (MM_OPT_TRAVERSAL -1): the certified grid search when the scene allows
// it (C3 ...), else the lean BVH loop (form 7) when every rect has a compact
// record, else form 5.
Choice choose_method(const SceneFacts& f, const PlanOptions& o) {
    const bool auto_form = o.opt_ww < 0;
    Choice c;
    c.form = auto_form ? (f.grid_ok ? kFormGrid : (f.lean_ok ? kFormLean : kFormLeafInterior)) : o.opt_ww;
    if (c.form == kFormGrid) {
        if (!f.grid_ok)
            return refuse<Choice>(MM_ERR_UNSUPPORTED, std::string("grid search unavailable for this scene: ") + f.grid_why);
        const bool slow = !f.lean_ok || f.grid_slow;  // general rect tests for the SLOW records
        // maze grids (one cell along y, compact records): only the maze forms read them
        if (f.grid_flat && slow) return refuse<Choice>(MM_ERR_UNSUPPORTED, "maze grid with SLOW records");
        if (slow) c.form = kFormGridSlow;
        if (f.grid_wide) c.form += kFormGridWide - kFormGrid;
        if (f.grid_flat) c.form += kFormGridFlat;
    } else if (c.form == kFormLean && !f.lean_ok) {
        return refuse<Choice>(MM_ERR_UNSUPPORTED, "loop form 7 needs compact records for every rect");
    }
    return c;
}

// The grid search in the placement that holds most of it in LDS; else the lean
// BVH loop (form 7) when the nodes + records fit LDS, else form 5 with the
// nodes in LDS when they fit, else through L1/L2.  MM_OPT_LDS_NODES 0 stages
// nothing.
Choice choose_placement(const SceneFacts& f, const PlanOptions& o, int form) {
    const size_t budget = kLdsPerBlock;
    const bool auto_form = o.opt_ww < 0;
    Choice c;
    c.form = form;
    if (form >= kFormGrid) {
        auto grid = [&](int m) {
            if (!wavepersist_built(m, form))
                return refuse<Choice>(MM_ERR_UNSUPPORTED, "grid form " + std::to_string(form) +
                                                              " not built for LDS mode " + std::to_string(m));
            c.mode = m;
            return c;
        };
        // the static-grid placements stage into the kernel's static grid array: their images must fit its capacity
        const size_t cap = wavepersist_grid_cap(0);
        if (f.grid_wide)  // built only when the whole image fits that capacity (grid_build.cpp)
            return grid(o.opt_lds && f.bytes <= cap ? kLdsGridImage : kLdsGridNone);
        if (o.opt_lds && f.bytes <= cap) return grid(kLdsGridImage);
        // compact records + class table + index (N=64: ~77 KB), leaf boxes global
        if (o.opt_lds && f.grid_flat && f.off_box <= cap) return grid(kLdsGridData);
        if (o.opt_lds && f.off_data <= budget) return grid(kLdsGridIndex);
        if (!auto_form || !o.opt_lds) return grid(kLdsGridNone);
        // the index does not fit LDS: auto takes the BVH (nodes in LDS or cached), which is not
        // measured against the all-global grid
        c.form = f.lean_ok ? kFormLean : kFormLeafInterior;
    }
    // nodes + records in LDS (lean form 7 or form 5), nodes only (form 5), or nothing
    if (o.opt_lds && o.opt_lds_rects && lds_stage_bytes(f, kLdsNodesRecs) <= budget) {
        c.mode = kLdsNodesRecs;
    } else {
        if (c.form == kFormLean && !auto_form)
            return refuse<Choice>(MM_ERR_UNSUPPORTED,
                                  "loop form 7 needs the BVH nodes + compact records in LDS (its other placements "
                                  "measured slower and were removed, DESIGN.md §4)");
        c.form = kFormLeafInterior;
        c.mode = (o.opt_lds && lds_stage_bytes(f, kLdsNodes) <= budget) ? kLdsNodes : kLdsNone;
    }
    return c;
}

// A path of bounce_limit b reads b - 1 direction samples when it meets no mirror (its last bounce reads
// none), 1.91 trials each at acceptance pi / 6, and a wave runs a round in the bounce whenever one of its 64
// lanes has run out.  The wave model (scripts/predraw_model.py, profiles/predraw/model.txt) puts the cheapest
// pre-pass at bounce_limit 8 near 22 trials with a flat minimum, and C3 measured fastest at 24 (1.865 ms/frame;
// 20: 1.881, 28: 1.897, 16: 1.932, 31: 1.931, 0: 2.058 -- profiles/predraw/ab_k_sweep.txt): 3 b, capped by
// the window's 31.
//
// With the pooled top-up rounds (MM_OPT_PREDRAW_POOL, mm_trace.h pool_trials) the own rounds no longer pay
// for the unluckiest of 64 lanes: they stop near the mean need and the pooled rounds serve the lanes still
// short, each with a power-of-two share of the wave's lanes.  Below the mean most lanes are still short and
// a share is one lane -- an own round at the pooled round's price (scripts/predraw_pool_model.py,
// profiles/pool/model.txt: cheapest at bounce_limit 8 at 13..14 own rounds, 16 within 1 %, 12 within 4 %):
// 2 (b - 1), the mean need rounded up (C3 measured: 13, 14, 16 and 18 within 0.5 % of each other, 12 0.7 %
// and 10 2.3 % slower, profiles/pool/ab.txt).  The pooled rounds only fill the window's 31: past b = 13 the
// mean need leaves them under 7 trials of room, the model's gain is gone by b = 16 (the N = 64 scene
// measured 0.9 % slower at 30 own rounds), and the own rounds fill the window as before.
uint32_t plan_predraw(int opt_predraw, bool pool, uint32_t bounce_limit) {
    if (opt_predraw >= 0) return std::min<uint32_t>((uint32_t)opt_predraw, 31u);
    const uint64_t mean2 = 2ull * (bounce_limit ? bounce_limit - 1u : 0u);
    if (pool && mean2 <= 24u) return (uint32_t)mean2;
    return (uint32_t)std::min<uint64_t>(3ull * bounce_limit, 31u);
}
// The accepted trials the pooled rounds top a window up to: what the path reads, b - 1 (its last bounce reads
// none), at most the window's 31.  0: no pooled rounds.
uint32_t plan_predraw_pool(bool pool, uint32_t bounce_limit) {
    if (!pool || bounce_limit < 2u) return 0u;
    return std::min<uint32_t>(bounce_limit - 1u, 31u);
}

LaunchPlan plan_tile(const SceneFacts& f, const PlanOptions& o, int form, int mode, const size_t static_lds[2],
                     const mm_ext& e, uint32_t w, uint32_t h, uint32_t n_frames, const char* multi_fn) {
    const bool multi = multi_fn != nullptr;
    const std::string fn = multi ? multi_fn : "";
    const uint64_t row_paths = (uint64_t)w * e.spp;
    const uint64_t tile_paths = row_paths * h;
    // MM_PIPE_WAVEFRONT: the wave-persistent kernel with mirror-tail deferral (compaction) always on
    const bool wave = o.pipe == MM_PIPE_WAVEFRONT;
    const bool persist = o.pipe != MM_PIPE_REFERENCE && (wave || o.opt_persist == 2);
    // mirror-tail deferral (MM_OPT_DEFER): samples staged per path, tails run from block-local rings; built for
    // the grid search and the lean BVH form with records in LDS (other forms run without it).  Auto: with the
    // whole search structure in LDS (the maze grid with its leaf boxes, or BVH nodes + compact records) and paths
    // of >= 8 bounces, on launches of >= MM_OPT_DEFER_MIN paths (C3 20 frames per launch 2.64 vs 2.74 ms/frame,
    // C4 20.97 vs 21.80, profiles/r03/ab_defer_claims.txt; rank 0 of an 8-way C3 split, 41 M paths per launch,
    // 0.356 vs 0.362, profiles/r03/emulated_scaling/; the N=64 scene, leaf boxes via L1/L2: 5.23 vs 4.90 without),
    // or where the samples are staged anyway (64 % spp != 0)
    const bool defer_on =
        o.opt_defer > 0 ||
        (o.opt_defer < 0 && ((lds_whole_search(mode) && e.bounce_limit >= 8u) ||
                             ((lds_whole_search(mode) || mode == kLdsGridData) && 64 % e.spp != 0)));
    const bool defer_built = persist && wavepersist_defer_built(mode, form);
    if (wave && !defer_built)
        return refuse<LaunchPlan>(MM_ERR_UNSUPPORTED,
                                  "MM_PIPE_WAVEFRONT: no tail-deferral kernel for this scene's query "
                                  "method / LDS placement (grid search, or BVH form 7 with nodes + "
                                  "records in LDS)");
    LaunchPlan p;
    p.predraw = plan_predraw(o.opt_predraw, o.opt_predraw_pool, e.bounce_limit);
    p.predraw_pool = plan_predraw_pool(o.opt_predraw_pool, e.bounce_limit);
    p.defer = defer_built && (defer_on || wave) && (wave || tile_paths * n_frames >= o.opt_defer_min);
    // the deferral kernel's static LDS (tail ring, claimed queue ranges, and with ring kind 2 the rings'
    // 32 KB of records) must leave two 1024-thread blocks per CU: the records go to LDS where the
    // image leaves room (C3: 44 KB + 34 KB), else to global memory; a grid image without room even for the
    // ring words runs without the rings
    if (p.defer) {
        const size_t img = lds_stage_bytes(f, mode);
        for (int kind : {2, 1}) {
            const size_t st = static_lds[kind - 1];
            // (static grid: the image goes into the kernel's static array)
            if (st != kNotBuilt && (lds_static_grid(mode) ? img <= wavepersist_grid_cap(kind) : img + st <= kLdsPerBlock)) {
                p.ring = kind;
                break;
            }
        }
        if (!p.ring) {
            if (wave)
                return refuse<LaunchPlan>(MM_ERR_UNSUPPORTED,
                                          "MM_PIPE_WAVEFRONT: grid image + tail ring exceed the LDS budget");
            p.defer = false;
        }
    }
    const bool fusable = persist && o.opt_fuse && 64 % e.spp == 0;
    // staging bound: a multi-frame launch stages all its frames at once; past kStagePathsMax it runs without
    // the rings (fused resolve) if it can
    if (p.defer && multi && tile_paths * n_frames > kStagePathsMax && fusable && !wave) p.defer = false;
    if (!p.defer) p.ring = 0;
    // wave-persistent kernel with whole pixels per 64-path chunk: resolve fused
    p.fuse = fusable && !p.defer;
    // Rows per launch: the fused resolve needs no staging (one launch covers up to 2^31 paths, a whole C5
    // frame); staged samples (tail deferral, or no fused resolve) are bounded by kStagePathsMax per launch
    // (64 Mi paths without deferral, where the non-persistent kernels' short launches lose nothing)
    const uint64_t batch_paths = p.fuse ? (1ull << 31) : p.defer ? kStagePathsMax : (64ull << 20);
    p.rows_per_batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(h, batch_paths / row_paths));
    if (row_paths * p.rows_per_batch > 0xFFFFFFFFull)
        return refuse<LaunchPlan>(MM_ERR_INVALID, "mm_trace_tile: row too large");
    if (multi) {
        // several frames in one launch: the wave-persistent kernel's queue, with the fused resolve or
        // (tail deferral) samples staged per frame
        if (!p.fuse && !p.defer)
            return refuse<LaunchPlan>(MM_ERR_UNSUPPORTED, fn + ": needs the wave-persistent kernel with the "
                                                               "fused resolve (64 % spp == 0) or tail deferral");
        if (e.flags & MM_EXT_ACCUMULATE)
            return refuse<LaunchPlan>(MM_ERR_INVALID, fn + ": frames of one launch cannot accumulate into one image");
        const uint64_t queue = ((tile_paths + 63) / 64) * 64 * n_frames;
        if (queue + (1ull << 24) > 0xFFFFFFFFull)
            return refuse<LaunchPlan>(MM_ERR_INVALID, fn + ": more paths than one launch holds (2^32)");
        if (p.defer && tile_paths * n_frames > kStagePathsMax)
            return refuse<LaunchPlan>(MM_ERR_INVALID, fn + ": the frames' staged samples exceed 6 GiB (2^29 paths) per "
                                                           "launch; use fewer frames per launch");
        if (p.rows_per_batch < h) return refuse<LaunchPlan>(MM_ERR_INVALID, fn + ": tile too large for one launch");
    }
    return p;
}

namespace {

// One list of n entries in one launch of the plain body's list instances: plan_pixels' and plan_rays' rule.
// name: the call's; a_list / the_list: how its texts speak of the list.
LaunchPlan plan_one_list(const std::string& name, const char* a_list, const char* the_list, const PlanOptions& o,
                         const mm_ext& e, uint64_t n) {
    if (o.pipe == MM_PIPE_WAVEFRONT)
        return refuse<LaunchPlan>(MM_ERR_UNSUPPORTED, name + ": MM_PIPE_WAVEFRONT runs the tail rings, which " +
                                                          a_list + " never does");
    const bool persist = o.pipe != MM_PIPE_REFERENCE && o.opt_persist == 2;
    // (n < 2^63 / 4096 first: the product below cannot wrap)
    if (n > 0xFFFFFFFFull || e.spp == 0)
        return refuse<LaunchPlan>(MM_ERR_INVALID, name + ": more paths than one launch holds (2^32)");
    const uint64_t paths = n * e.spp;
    const uint64_t queue = ((paths + 63) / 64) * 64;
    if (queue + (1ull << 24) > 0xFFFFFFFFull)
        return refuse<LaunchPlan>(MM_ERR_INVALID, name + ": more paths than one launch holds (2^32)");
    LaunchPlan p;
    p.predraw = plan_predraw(o.opt_predraw, o.opt_predraw_pool, e.bounce_limit);
    p.predraw_pool = plan_predraw_pool(o.opt_predraw_pool, e.bounce_limit);
    p.fuse = persist && o.opt_fuse && 64 % e.spp == 0;
    p.rows_per_batch = 1;
    if (!p.fuse && paths > kStagePathsMax)
        return refuse<LaunchPlan>(MM_ERR_INVALID, name + ": " + the_list + "'s staged samples exceed 6 GiB (2^29 "
                                                      "paths); use a shorter list");
    return p;
}

}  // namespace

LaunchPlan plan_pixels(const PlanOptions& o, const mm_ext& e, uint64_t n_pixels) {
    return plan_one_list("mm_trace_pixels", "a pixel list", "the list", o, e, n_pixels);
}

LaunchPlan plan_rays(const PlanOptions& o, const mm_ext& e, uint64_t n_rays) {
    return plan_one_list("mm_trace_rays", "a ray list", "the ray list", o, e, n_rays);
}

int lists_total(const uint64_t* offsets, uint32_t n_lists, uint64_t& total, std::string& error) {
    total = 0;
    error.clear();
    if (n_lists == 0 || n_lists > 65535u) error = "mm_trace_pixel_lists: n_lists outside 1..65535";
    else if (!offsets) error = "mm_trace_pixel_lists: null offsets";
    else if (offsets[0] != 0) error = "mm_trace_pixel_lists: offsets[0] is not 0";
    else
        for (uint32_t f = 0; f < n_lists && error.empty(); ++f)
            if (offsets[f + 1] < offsets[f]) error = "mm_trace_pixel_lists: offsets decrease";
    if (!error.empty()) return MM_ERR_INVALID;
    total = offsets[n_lists];
    return MM_OK;
}

ListsPlan plan_pixel_lists(const PlanOptions& o, const mm_ext& e, const uint64_t* offsets, uint32_t n_lists) {
    ListsPlan r;
    auto refuse_with = [&](int code, const std::string& why) {
        r.plan.code = code;
        r.plan.error = why;
        r.lists.clear();
        return r;
    };
    if (o.pipe == MM_PIPE_WAVEFRONT)
        return refuse_with(MM_ERR_UNSUPPORTED, "mm_trace_pixel_lists: MM_PIPE_WAVEFRONT runs the tail rings, which a "
                                               "pixel list never does");
    std::string why;
    if (int rc = lists_total(offsets, n_lists, r.n_entries, why)) return refuse_with(rc, why);
    const char* too_many = "mm_trace_pixel_lists: more paths than one launch holds (2^32)";
    // (n_entries < 2^63 / 4096 first: no product below can wrap)
    if (r.n_entries > 0xFFFFFFFFull || e.spp == 0) return refuse_with(MM_ERR_INVALID, too_many);
    const bool persist = o.pipe != MM_PIPE_REFERENCE && o.opt_persist == 2;
    uint64_t chunks = 0;  // at most 2^32 * 4096 / 64 + 65535
    r.lists.resize(n_lists);
    for (uint32_t f = 0; f < n_lists; ++f) {
        const uint64_t n = offsets[f + 1] - offsets[f], paths = n * e.spp;
        ListSpan& l = r.lists[f];
        // (values past 32 bits are refused below, before anything reads the spans)
        l.first_chunk = (uint32_t)chunks;
        l.n_chunks = (uint32_t)((paths + 63) / 64);
        l.first_entry = (uint32_t)offsets[f];
        l.n_entries = (uint32_t)n;
        l.n_paths = (uint32_t)paths;
        chunks += (paths + 63) / 64;
    }
    if (chunks * 64 + (1ull << 24) > 0xFFFFFFFFull) return refuse_with(MM_ERR_INVALID, too_many);
    r.n_chunks = (uint32_t)chunks;
    r.plan.predraw = plan_predraw(o.opt_predraw, o.opt_predraw_pool, e.bounce_limit);
    r.plan.predraw_pool = plan_predraw_pool(o.opt_predraw_pool, e.bounce_limit);
    r.plan.fuse = persist && o.opt_fuse && 64 % e.spp == 0;
    r.plan.rows_per_batch = 1;
    if (!r.plan.fuse && r.n_entries * e.spp > kStagePathsMax)
        return refuse_with(MM_ERR_INVALID, "mm_trace_pixel_lists: the lists' staged samples exceed 6 GiB (2^29 paths); "
                                           "use shorter lists");
    return r;
}

}  // namespace mm

// The build's instance lists (mm_variants.h) as the C ABI tells them: ring kinds 1 and 2 where the pair has a
// tail-deferral variant.
extern "C" int mm_variant_built(int lds_mode, int form, int ring) {
    if (ring == 0) return mm::wavepersist_built(lds_mode, form) ? 1 : 0;
    return (ring == 1 || ring == 2) && mm::wavepersist_defer_built(lds_mode, form) ? 1 : 0;
}
