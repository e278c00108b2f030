// mm_variants.h — which kernel variants the build holds, written once: the query
// forms, the LDS placements and their budget, and the (placement, form) lists
// that trace_kernels.hip and aov_kernels.hip instantiate.  Plain C++ with no
// device code, so the launch policy (mm_plan.cpp) and its CPU test read the
// same lists the kernels are built from.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mm {

// Diagnostics build (-DMM_LANE_STATS, scripts/lane_probe.py): per phase of the
// bounce loop, the wave-iterations that run it and the lanes active in them,
// counted in block-local LDS words and added to the wave-timeline buffer at
// exit.  Not a product build: the counting perturbs the timing.
enum LanePhase : int {
    kLpChunk, kLpBounce, kLpGlobal, kLpGridIter, kLpRectTest, kLpCellStep, kLpCert, kLpFallback,
    kLpShade, kLpDiffuse, kLpTrial, kLpMirror, kLpCertFull, kLpPredraw, kLpPool, kLpCount
};

// Closest-hit query methods of the wave-persistent kernel (MM_OPT_TRAVERSAL):
// BVH loop forms (mm_trace.h) and the certified grid search (mm_grid.h).
// kFormGridSlow (internal): the grid search on a scene with SLOW rect records.
// kFormGridWide / kFormGridWideSlow (internal): the same on a grid with 64-bit
// cell words (per-face list ranges; grid_build.cpp).
// kFormGridFlat (internal, + kFormGrid..kFormGridWideSlow): the same on a grid
// with one cell along y (the walk steps x / z only; mm_grid.h kFlat).
enum : int {
    kFormIfIf = 0, kFormLeafInterior = 5, kFormLean = 7,
    kFormGrid = 11, kFormGridSlow = 12, kFormGridWide = 13, kFormGridWideSlow = 14,
    kFormGridFlat = 4  // offset: 15..18
};

// LDS placements (what a resident block of the wave-persistent kernel stages
// before tracing; the rest is read through L1/L2).  MM_INFO_LAST_LDS_MODE
// reports the numbers.
enum LdsMode : int {
    kLdsNone = 0,        // nothing (nodes, records global)            BVH form 5
    kLdsNodes = 1,       // BVH nodes                                   BVH form 5 (general rect test)
    kLdsNodesRecs = 3,   // BVH nodes + compact slot records            BVH forms 5 / 7
    kLdsGridImage = 11,  // the whole grid image                        grid search
    kLdsGridIndex = 12,  // grid cells + lists, records + boxes global  grid search
    kLdsGridNone = 13,   // nothing (the grid image global)             grid search
    kLdsGridData = 14,   // grid records + class table + cells + lists, leaf boxes global (the maze forms)
};
// kLdsGridImage / kLdsGridData stage into the kernel's static grid array (trace_kernels.hip stage_and_run);
// the other placements use dynamic LDS beside the kernel's static words.
constexpr bool lds_static_grid(int mode) { return mode == kLdsGridImage || mode == kLdsGridData; }
// The whole search structure in LDS (the placements tail deferral is measured on, mm_plan.cpp).
constexpr bool lds_whole_search(int mode) { return mode == kLdsGridImage || mode == kLdsNodesRecs; }

// Bytes a placement stages: BVH nodes are 2 x float4, compact slot records 5 x uint2; the grid image's
// sections are [index: cells + lists | data at off_data: class table, records | windows at off_box]
// ("boxes" below: the 24 B per rect at off_box, the fast certificate's windows; the leaf boxes are never staged).
constexpr size_t lds_stage_bytes(int mode, uint32_t n_nodes, uint32_t n_rects, uint32_t grid_bytes,
                                 uint32_t grid_off_data, uint32_t grid_off_box) {
    switch (mode) {
        case kLdsGridImage: return grid_bytes;
        case kLdsGridIndex: return grid_off_data;
        case kLdsGridData: return grid_off_box;
        case kLdsNodes: return 32 * (size_t)n_nodes;
        case kLdsNodesRecs: return 32 * (size_t)n_nodes + 40 * (size_t)n_rects;
        default: return 0;
    }
}

// 1024-thread blocks at 8 waves per SIMD -> two blocks per CU -> 80 KB of LDS each.
constexpr uint32_t kLdsPerBlock = 80 * 1024;

// Tail ring entries per resident block (mm_launch.h TailQueue).
constexpr uint32_t kTailRing = 512;
// Words per wave of the claimed queue range (trace_kernels.hip claim_words).
#ifdef MM_TAIL_CLOCKS
constexpr uint32_t kClaimWords = 16;
#else
constexpr uint32_t kClaimWords = 2;
#endif

// Capacity of the static grid array: what the block's 80 KB leave after the
// kernel's other static LDS.  kRing: 0 no tail deferral, 1 tail rings with
// global records, 2 tail rings with their records in LDS.
template <int kRing>
constexpr uint32_t grid_lds_cap() {
    uint32_t other = kClaimWords * 16u * 4u + 64u;  // claimed queue ranges + alignment slack
    if (kRing != 0) other += (4u + kTailRing) * 4u;  // ring counters and turn words
    if (kRing == 2) other += 4u * kTailRing * 16u;   // ring payload
#ifdef MM_LANE_STATS
    other += 2u * kLpCount * 4u;
#endif
    return (kLdsPerBlock - other) & ~15u;
}
constexpr uint32_t wavepersist_grid_cap(int ring) {
    return ring == 2 ? grid_lds_cap<2>() : ring == 1 ? grid_lds_cap<1>() : grid_lds_cap<0>();
}

// (LDS mode, form) pairs; the tail-deferral variant (MM_OPT_DEFER) is built
// for the grid search and the lean BVH form with records in LDS.  The build
// holds what MM_PIPE_AUTO can select: the grid search, and the BVH forms for
// scenes the grid cannot take (nodes + records in LDS, nodes only, nothing).
// (The A/B-only placements -- split node cache, nodes with global records,
// dictionary nodes, loop form 0 -- measured slower and were removed in round
// 6)  The maze forms (flat grid walk,
// compact records; grid_build.cpp decides) in every grid placement: a maze
// grid's compact records are read by no other form.  (No SLOW records in
// maze grids: no slow maze forms.)
#define MM_FLAT_INSTANCES(X)                                                                                  \
    X(11, kFormGridWide + kFormGridFlat) X(11, kFormGrid + kFormGridFlat) X(14, kFormGrid + kFormGridFlat)     \
    X(12, kFormGrid + kFormGridFlat) X(13, kFormGridWide + kFormGridFlat) X(13, kFormGrid + kFormGridFlat)
#define MM_DEFER_INSTANCES(X)                                                                                 \
    X(11, kFormGrid) X(12, kFormGrid) X(13, kFormGrid)                                                        \
    X(11, kFormGridSlow) X(12, kFormGridSlow) X(13, kFormGridSlow)                                            \
    X(11, kFormGridWide) X(13, kFormGridWide) X(11, kFormGridWideSlow) X(13, kFormGridWideSlow)               \
    MM_FLAT_INSTANCES(X) X(3, kFormLean)
// the variants without a tail-deferral build
#define MM_PLAIN_INSTANCES(X) X(0, kFormLeafInterior) X(1, kFormLeafInterior) X(3, kFormLeafInterior)
#define MM_WP_INSTANCES(X) MM_DEFER_INSTANCES(X) MM_PLAIN_INSTANCES(X)

// Whether the tail-deferral variant / any variant exists for this (LDS mode, form).
constexpr bool wavepersist_defer_built(int lds_mode, int form) {
#define MM_WP(L, F) if (lds_mode == (L) && form == (F)) return true;
    MM_DEFER_INSTANCES(MM_WP)
    return false;
}
constexpr bool wavepersist_built(int lds_mode, int form) {
    if (wavepersist_defer_built(lds_mode, form)) return true;
    MM_PLAIN_INSTANCES(MM_WP)
#undef MM_WP
    return false;
}

// Query policy of the batch-query / feature-buffer kernels (aov_kernels.hip):
// the method MM_OPT_TRAVERSAL / the scene select (mm_runtime.hip aov_policy),
// always over the global-memory views (grid placement 13, BVH placement 0:
// profiles/aov/ab.txt).
enum AovPolicy : int {
    kAovRef = 0,        // MM_PIPE_REFERENCE: RefQuery
    kAovBvhLi = 1,      // BVH loop form 5
    kAovBvhLean = 2,    // BVH loop form 7 (compact records)
    kAovGrid = 3,       // + kAovGridSlow | kAovGridWide | kAovGridFlat: the certified grid search
    kAovGridSlow = 1, kAovGridWide = 2, kAovGridFlat = 4,
};
// The instances: the reference walk, the two BVH forms, and the grid search's
// slow / wide / flat forms (no slow maze form: choose_method's rule).
#define MM_AOV_POLICIES(X)                                                                                   \
    X(kAovRef) X(kAovBvhLi) X(kAovBvhLean) X(kAovGrid) X(kAovGrid + kAovGridSlow) X(kAovGrid + kAovGridWide) \
    X(kAovGrid + kAovGridWide + kAovGridSlow) X(kAovGrid + kAovGridFlat) X(kAovGrid + kAovGridFlat + kAovGridWide)
constexpr bool aov_policy_built(int policy) {
#define MM_AOV(P) if (policy == (P)) return true;
    MM_AOV_POLICIES(MM_AOV)
#undef MM_AOV
    return false;
}

}  // namespace mm
