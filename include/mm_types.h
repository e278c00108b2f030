/*
 * mm_types.h — plain-old-data types shared by the HIP path (mm_api.h) and the
 * host scene builder (mm_scene.h).
 *
 * Every struct is byte-identical to the reference's `#[repr(C)]` Rust type and
 * to the Metal struct the kernel reads, so a Rust host could pass its own
 * `Vec<Plane>` / `Vec<BVHNode>` / `Uniform` straight through an `extern "C"`
 * block.  Sizes and offsets are pinned by static asserts in
 * mirror-maze_amd/csrc/mm_layout_check.cpp and by tests/test_layout.py.
 */
#ifndef MM_TYPES_H
#define MM_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == Plane   (src/main.rs:51-58)   == rect     (src/shaders.metal:19-24)
 *    origin, side v, side u, albedo; packed_float3 x 4 = 48 B               */
typedef struct mm_rect {
    float o[3];
    float v[3];
    float u[3];
    float color[3];
} mm_rect;

/* == BVHNode (src/main.rs:74-81)   == bvh_node (src/shaders.metal:30-35)
 *    count > 0: leaf covering idx[left_first .. left_first+count)
 *    count = 0: interior node, children at left_first and left_first+1       */
typedef struct mm_node {
    float mn[3];
    float mx[3];
    uint32_t left_first;
    uint32_t count;
} mm_node;

/* == Camera  (src/main.rs:32-39)   == camera   (src/shaders.metal:37-42)
 *    quat is (x, y, z, w)                                                    */
typedef struct mm_camera {
    float center[3];
    float focal;
    float quat[4];
    float viewport[2];
} mm_camera;

/* == Uniform (src/main.rs:41-49)   == uni      (src/shaders.metal:237-243)  */
typedef struct mm_uniform {
    mm_camera cam;
    float view_w;
    float view_h;
    uint32_t chunk_w;
    uint32_t time;
} mm_uniform;

/* Throughput-mode extension.  The reference hard-codes these inside the
 * kernel (src/shaders.metal:293-296, "TODO: uniform this"); the offline
 * renderer lifts them into a uniform.                                        */
typedef struct mm_ext {
    uint32_t spp;           /* samples per pixel (reference: 64)              */
    uint32_t bounce_limit;  /* reference: 5   (shaders.metal:294)             */
    uint32_t mirror_limit;  /* reference: 15  (shaders.metal:295)             */
    uint32_t frame;         /* RNG key; plays the role of uni.time            */
    uint32_t flags;         /* MM_EXT_* bits                                   */
    uint32_t reserved;
} mm_ext;

/* mm_ext.flags */
#define MM_EXT_COUNT_STATS   0x1u  /* fill mm_stats (costs a few %)            */
#define MM_EXT_ACCUMULATE    0x2u  /* out += frame value instead of out = ...  */
#define MM_EXT_RGBA8         0x4u  /* out holds RGBA8 (4 B per pixel: the texture-write
                                      conversion of mm_quantize_rgba8, alpha 255)
                                      instead of float4; not with ACCUMULATE    */

/* Work counters.  A "ray" is one closest-hit BVH query, i.e. one execution
 * of src/shaders.metal:307.                                  */
typedef struct mm_stats {
    uint64_t rays;          /* intersect_bvh_iterative calls                  */
    uint64_t node_visits;   /* interior nodes expanded (2 AABB tests each)    */
    uint64_t rect_tests;    /* ray_rect_intersect calls                       */
    uint64_t paths;         /* samples traced                                 */
} mm_stats;

/* Feature buffers of mm_trace_aov (mm_api.h): three optional DEVICE pointers,
 * each NULL or n_frames * w * h elements, frame-major, row-major over the
 * tile.  normal_depth and albedo hold float4 (16-byte aligned), id uint32.   */
typedef struct mm_aov {
    float*    normal_depth; /* (side * n, distance along the mirror chain)    */
    float*    albedo;       /* (rect colour, mirror hits before the surface)  */
    uint32_t* id;           /* rect index | kind << 30, MM_AOV_ID_*           */
} mm_aov;

/* mm_aov.id and mm_query_rays' k */
#define MM_AOV_ID_MISS       0xFFFFFFFFu  /* nothing hit                        */
#define MM_AOV_ID_FAILED     0xFFFFFFFEu  /* no answer: the call reports MM_ERR_STACK */
#define MM_AOV_ID_SURFACE    0x40000000u  /* | k: a surface that shades diffusely */
#define MM_AOV_ID_MIRROR_END 0x80000000u  /* | k: a mirror's front, mirror_limit reached */
#define MM_AOV_ID_RECT       0x00FFFFFFu  /* mask of k                          */

/* Parameters of mm_denoise_frames (mm_api.h): the edge-aware a-trous filter
 * over a traced frame, guided by the mm_aov buffers of the same tile. */
#define MM_DENOISE_MAX_PASSES 8
#define MM_DN_RGBA8 1u   /* the output is RGBA8 (4 B per pixel), not float4   */
typedef struct mm_denoise_params {   /* 16 bytes */
    uint32_t n_passes;  /* 1..MM_DENOISE_MAX_PASSES; pass i spaces its taps 2^i apart */
    float    sigma_z;   /* depth term; <= 0: off */
    float    sigma_l;   /* luminance term of pass 0, halved every pass; <= 0: off */
    uint32_t flags;     /* MM_DN_RGBA8 */
} mm_denoise_params;

/* Parameters of mm_denoise_frames_var (mm_api.h): the same filter with its
 * luminance stop scaled per pixel by the standard deviation of the pixel mean. */
#define MM_DNV_RGBA8 1u   /* the output is RGBA8 (4 B per pixel), not float4  */
typedef struct mm_denoise_var_params {   /* 24 bytes */
    uint32_t n_passes;  /* 1..MM_DENOISE_MAX_PASSES; pass i spaces its 5x5 taps 2^i apart */
    float    sigma_z;   /* depth term; <= 0: off (as mm_denoise_params) */
    float    sigma_l;   /* luminance stop in standard deviations; <= 0: off.  NOT halved per pass */
    float    eps_l;     /* added to the stop; finite and > 0 when sigma_l > 0, else ignored */
    uint32_t flags;     /* MM_DNV_RGBA8 */
    uint32_t reserved;  /* 0 */
} mm_denoise_var_params;

/* Parameters of mm_accumulate_frames (mm_api.h): temporal accumulation of a
 * camera sequence's frames, the history reprojected through the mirror chains. */
typedef struct mm_temporal_params {   /* 16 bytes */
    uint32_t n_max;   /* 1..65535: history length cap (blend factor 1/min(N, n_max)) */
    float    tol_z;   /* > 0: relative distance tolerance of a history tap */
    float    w_min;   /* in (0, 1]: least sum of valid bilinear weights that counts as history */
    uint32_t flags;   /* 0 */
} mm_temporal_params;

typedef struct mm_temporal_prev {     /* the frame before frame 0, from an earlier call */
    const float* color;   /* DEVICE, w*h float4: an earlier call's out frame (alpha = N) */
    mm_aov       guides;  /* DEVICE, that frame's three buffers (one frame), all required */
    mm_camera    cam;     /* that frame's camera */
} mm_temporal_prev;

typedef struct mm_temporal_prev_var { /* 80 bytes: mm_temporal_prev for mm_accumulate_frames_var */
    const float* color;   /* DEVICE, w*h float4: an earlier call's out frame (alpha = N) */
    mm_aov       guides;  /* DEVICE, that frame's three buffers (one frame), all required */
    mm_camera    cam;     /* that frame's camera */
    const float* var;     /* DEVICE, w*h floats: that frame's var_out of the earlier call */
} mm_temporal_prev_var;

/* Parameters of mm_upsample_frames (mm_api.h): frames traced on the lattice of
 * every scale-th pixel, rebuilt at full resolution from the mm_aov buffers. */
typedef struct mm_upsample_params {   /* 16 bytes */
    uint32_t scale;     /* 2, 4 or 8: the lattice holds window pixels (scale*X, scale*Y) */
    float    w_min;     /* in (0, 1]: least sum of valid bilinear weights that counts; below it the pixel is a hole */
    uint32_t flags;     /* 0 */
    uint32_t reserved;  /* 0 */
} mm_upsample_params;

/* Return codes (0 = success; never panics or throws across the ABI). */
#define MM_OK               0
#define MM_ERR_INVALID     -1  /* bad argument / shape                        */
#define MM_ERR_HIP         -2  /* HIP runtime error (message in last_error)   */
#define MM_ERR_NOMEM       -3
#define MM_ERR_NO_SCENE    -4  /* trace before upload                          */
#define MM_ERR_STACK       -5  /* BVH deeper than the 50-entry stack           */
#define MM_ERR_UNSUPPORTED -6  /* geometry the kernel does not implement       */

#ifdef __cplusplus
}
#endif
#endif /* MM_TYPES_H */
