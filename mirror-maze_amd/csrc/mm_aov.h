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

// (Query policies of the two kernels, enum AovPolicy, and aov_policy_built: mm_variants.h.)

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
