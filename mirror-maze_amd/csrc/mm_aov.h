// mm_aov.h — host-callable launchers of aov_kernels.hip: the batch closest-hit
// query (mm_query_rays) and the per-pixel feature buffers (mm_trace_aov).
#pragma once

#include <hip/hip_runtime.h>

#include "mm_device.h"

namespace mm {

// A query's answer (8 B): the (t, k) the reference walk ends with.
struct RayHit {
    float t;
    uint32_t k;
};
constexpr uint32_t kHitMiss = 0xFFFFFFFFu;    // nothing hit: (1e30f, kHitMiss)
constexpr uint32_t kHitFailed = 0xFFFFFFFEu;  // the traversal stack overflowed (error bit kErrStack)
// id buffer: k | kind << 30 (k < 2^24, mm_upload_scene)
constexpr uint32_t kAovSurface = 1u << 30, kAovMirrorEnd = 2u << 30;

// Query policy of the two kernels: the method MM_OPT_TRAVERSAL / the scene
// select (mm_runtime.hip aov_policy), always over the global-memory views
// (grid placement 13, BVH placement 0: profiles/aov/ab.txt).
enum AovPolicy : int {
    kAovRef = 0,        // MM_PIPE_REFERENCE: RefQuery
    kAovBvhLi = 1,      // BVH loop form 5
    kAovBvhLean = 2,    // BVH loop form 7 (compact records)
    kAovGrid = 3,       // + kAovGridSlow | kAovGridWide | kAovGridFlat: the certified grid search
    kAovGridSlow = 1, kAovGridWide = 2, kAovGridFlat = 4,
};
bool aov_policy_built(int policy);

struct AovJob {
    mm_uniform u;
    const float* cams;  // null: u.cam; else camera record f (kCamStride floats) for frame f
    uint32_t n_frames, mirror_limit;
    uint32_t x0, y0, w, h, y_stride;
    float4* normal_depth;  // each null or n_frames * w * h elements
    float4* albedo;
    uint32_t* id;
};

hipError_t launch_query_rays(const DevScene& sc, int policy, const float4* rays, uint64_t n_rays, RayHit* hits,
                             uint32_t* err, hipStream_t s);
hipError_t launch_trace_aov(const DevScene& sc, int policy, const AovJob& job, uint32_t* err, hipStream_t s);
// Largest n_rays / w * h * n_frames one launch takes (a 31-bit block index).
uint64_t aov_max_items();

}  // namespace mm
