// aov_kernels.hip — gfx950 kernels that return closest-hit answers to the caller.
//
//   k_query_rays   mm_query_rays: one lane per caller-supplied ray, the (t, k)
//                  the reference walk ends with (intersect_bvh_iterative,
//                  shaders.metal:115-156, started at t = 1e30)
//   k_trace_aov    mm_trace_aov: one lane per pixel, the deterministic part of
//                  the path of its centre ray -- through the mirror chain
//                  (shaders.metal:326-330: reflect, no random draw) to the first
//                  surface that shades diffusely -- as normal + distance,
//                  albedo + mirror hits and primitive id
//
// Both run the query policies of mm_path.h (the certified grid search with the
// walk as fallback, the BVH loop forms, the straight reference walk) over the
// scene in global memory: a block traces one ray per lane, so staging the scene
// into LDS first would cost each block the whole image for 256 queries
// (profiles/aov/ab.txt).  A translation unit of its own: no
// instance of trace_kernels.hip is compiled differently for it.
#include <hip/hip_runtime.h>

#include <utility>

#include "grid_build.h"
#include "mm_aov.h"
#include "mm_launch.h"
#include "mm_path.h"

namespace mm {

constexpr uint32_t kAovThreads = 256;

// body(query) with the policy's query object over the global-memory views.
template <int kPolicy, typename F>
__device__ __forceinline__ void with_query(const DevScene& sc, F&& body) {
    if constexpr (kPolicy == kAovRef) {
        body(RefQuery<false>{sc});
    } else if constexpr (kPolicy == kAovBvhLi) {
        const auto v = view(sc.nodes);
        body(BvhQuery<false, kFormLeafInterior, decltype(v)>{sc, v});
    } else if constexpr (kPolicy == kAovBvhLean) {
        const auto v = view(sc.nodes, sc.recs);
        body(BvhQuery<false, kFormLean, decltype(v)>{sc, v});
    } else {
        constexpr int g = kPolicy - kAovGrid;
        const auto gv = grid_view(GlobalCells{reinterpret_cast<const char*>(sc.grid.cells)}, GlobalList{sc.grid.list},
                                  sc.grid.recs, sc.grid.box, sc.grid.cls);
        body(GridQuery<false, (g & kAovGridSlow) != 0, (g & kAovGridWide) != 0, (g & kAovGridFlat) != 0,
                       decltype(gv)>{sc, gv});
    }
}

// One closest-hit query from t = 1e30: true with (t, k) = the reference walk's
// answer ((kBig, kHitMiss) when nothing is hit), false when the traversal
// stack overflowed (no answer).
template <typename Q>
__device__ __forceinline__ bool closest_hit(const Q& q, F3 o, F3 d, bool hit_origin, float& t, uint32_t& k,
                                            ScratchStack& stack) {
    Counters c;
    t = kBig;
    k = kHitMiss;
    if (!q(o, d, hit_origin, t, k, stack, c)) return false;
    if (!(t < kBig)) k = kHitMiss;
    return true;
}

// rays: (o.xyz, .), (d.xyz, .) per ray, two 16-B loads per lane; hits: one 8-B store per lane.
template <int kPolicy>
__global__ __launch_bounds__(kAovThreads) void k_query_rays(DevScene sc, const float4* __restrict__ rays,
                                                            uint64_t n_rays, RayHit* __restrict__ hits,
                                                            uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * kAovThreads + threadIdx.x;
    if (i >= n_rays) return;
    const float4 o = rays[2 * i], d = rays[2 * i + 1];
    with_query<kPolicy>(sc, [&](const auto& q) {
        ScratchStack stack;
        RayHit h;
        // arbitrary rays: never "at a hit point", so the grid search checks its box
        if (!closest_hit(q, xyz(o), xyz(d), false, h.t, h.k, stack)) {
            atomicOr(err, kErrStack);
            h.t = kBig;
            h.k = kHitFailed;
        }
        hits[i] = h;
    });
}

// The camera of frame fr.  The record's address is wave-uniform (the frame
// comes from the block index), so through the constant address space its ten
// floats are scalar loads, as in the camera-sequence trace kernels.
__device__ __forceinline__ mm_camera frame_camera(const AovJob& job, uint32_t fr) {
    if (!job.cams) return job.u.cam;
    typedef const float __attribute__((address_space(4))) cam_float;
    cam_float* r = (cam_float*)(job.cams + (size_t)fr * kCamStride);
    mm_camera c;
    c.center[0] = r[0]; c.center[1] = r[1]; c.center[2] = r[2];
    c.focal = r[3];
    c.quat[0] = r[4]; c.quat[1] = r[5]; c.quat[2] = r[6]; c.quat[3] = r[7];
    c.viewport[0] = r[8]; c.viewport[1] = r[9];
    return c;
}

// Pixel `pix` of frame `fr` of the job's tile: the feature path of its centre ray, and the stores.
template <typename Q>
__device__ __forceinline__ void aov_pixel(const DevScene& sc, const Q& q, const AovJob& job, uint32_t fr,
                                          uint32_t pix, uint32_t n_pix, uint32_t* err) {
    mm_uniform u = job.u;
    u.cam = frame_camera(job, fr);
    const uint32_t j = pix / job.w, i = pix - j * job.w;
    const uint32_t px = job.x0 + i, py = job.y0 + j * job.y_stride;
    ScratchStack stack;
    F3 ori = F3{u.cam.center[0], u.cam.center[1], u.cam.center[2]};
    F3 dir = primary_dir(u, px, py);
    uint32_t mh = 0, id = kHitMiss;
    float dist = 0.0f, sg = 0.0f;
    // The loop carries the path only (ori, dir, mh, dist) and leaves with the result's id and the sign of
    // dot(dir, n) at the last hit; the buffers' values are formed after it.  (With the output values
    // assigned at the loop's exits they are loop-carried and undefined on entry, and this hipcc kept that
    // undefined copy for the lanes leaving at a mirror: their albedo came out as stale registers.)
    for (;;) {
        float t;
        uint32_t k;
        // (a ray after a mirror starts at a hit point: mm_path.h GridQuery)
        if (!closest_hit(q, ori, dir, mh != 0, t, k, stack)) {
            atomicOr(err, kErrStack);
            id = kHitFailed;
            break;
        }
        id = k;
        if (k == kHitMiss) break;
        // shade_step's classification of the hit (mm_trace.h): matte, or a mirror seen from behind, is lit
        const F3 nn = xyz(sc.geo[4 * k + 1]);
        sg = msign(dot3(dir, nn));
        dist = dist + t;
        const bool lit = sc.shade[2 * k].w == 0.0f || sg == 1.0f;
        if (lit || !(mh + 1 < job.mirror_limit)) {
            id = k | (lit ? kAovSurface : kAovMirrorEnd);
            break;
        }
        ori = ori + t * dir;                         // shade_step's mirror branch
        const float dd = dot3(nn, dir) * 2.0f;
        const F3 x = dir - dd * nn;
        dir = rsq(dot3(x, x)) * x;
        ++mh;
    }
    float4 nd = make_float4(0.0f, 0.0f, 0.0f, kBig);
    float4 al = make_float4(0.0f, 0.0f, 0.0f, (float)mh);
    if (id < kHitFailed) {  // SURFACE or MIRROR_END at rect k
        const uint32_t k = id & 0xFFFFFFu;
        const F3 nn = xyz(sc.geo[4 * k + 1]);
        const float4 s0 = sc.shade[2 * k];
        const float side = -sg;
        nd = make_float4(side * nn.x, side * nn.y, side * nn.z, dist);
        al = make_float4(s0.x, s0.y, s0.z, (float)mh);
    }
    const size_t o = (size_t)fr * n_pix + pix;
    if (job.normal_depth) job.normal_depth[o] = nd;
    if (job.albedo) job.albedo[o] = al;
    if (job.id) job.id[o] = id;
}


// Blocks [fr * bpf, (fr + 1) * bpf) hold frame fr's w * h pixels (the last one
// ragged), lane = pixel: each output's store is 16 B (4 B: id) per lane, coalesced.
template <int kPolicy>
__global__ __launch_bounds__(kAovThreads) void k_trace_aov(DevScene sc, AovJob job, uint32_t* err) {
    const uint32_t n_pix = job.w * job.h;
    const uint32_t bpf = (n_pix + kAovThreads - 1) / kAovThreads;
    const uint32_t fr = blockIdx.x / bpf;
    const uint32_t pix = (blockIdx.x - fr * bpf) * kAovThreads + threadIdx.x;
    if (pix >= n_pix) return;
    with_query<kPolicy>(sc, [&](const auto& q) { aov_pixel(sc, q, job, fr, pix, n_pix, err); });
}

#ifdef MM_AOV_AB_LDS
// A/B build only (profiles/aov/ab.txt; scripts/aov_bench.py with MIRROR_MAZE_LIB): the other scene placement
// for the maze grids -- trace_kernels.hip's LDS mode 11 -- as a persistent kernel, so that a block stages the
// grid image once and not once per 256 pixels: resident 1024-thread blocks, the whole image in (dynamic) LDS,
// each wave takes the 64-pixel chunks wave, wave + n_waves, ...  It measured slower than the global-memory
// views and is not part of the product build.
template <int kPolicy>
__global__ __launch_bounds__(1024) void k_trace_aov_lds(DevScene sc, AovJob job, uint32_t* err) {
    extern __shared__ uint4 aov_img[];
    constexpr int g = kPolicy - kAovGrid;
    constexpr bool kWide = (g & kAovGridWide) != 0, kFlat = (g & kAovGridFlat) != 0;
    // stage_and_run's mode 11: the data (class table, records, boxes) first, then cells (their first-entry
    // fields as LDS addresses) and lists
    const uint32_t d0 = sc.grid.off_data, nr16 = (sc.grid.bytes - d0) / 16u, ni16 = d0 / 16u;
    const uint4* src = sc.grid.image;
    for (uint32_t i = threadIdx.x; i < nr16; i += blockDim.x) aov_img[i] = src[ni16 + i];
    const uint32_t nc16 = sc.grid.off_list / 16u, lbase = lds_addr(aov_img + nr16) + sc.grid.off_list;
    for (uint32_t i = threadIdx.x; i < ni16; i += blockDim.x)
        aov_img[nr16 + i] = i < nc16 ? grid_stage_cells<kWide>(src[i], lbase) : src[i];
    __syncthreads();
    const char* base = reinterpret_cast<const char*>(aov_img);
    const char* index = base + 16u * nr16;
    const auto gv = grid_view(LdsCells{lds_addr(index)}, LdsList{lds_addr(index + sc.grid.off_list)},
                              reinterpret_cast<const uint4*>(base + (kFlat ? kGridClassBytes : 0u)),
                              reinterpret_cast<const float2*>(base + (sc.grid.off_box - d0)),
                              reinterpret_cast<const float4*>(base));
    const GridQuery<false, (g & kAovGridSlow) != 0, kWide, kFlat, decltype(gv)> q{sc, gv};
    const uint32_t n_pix = job.w * job.h, cpf = (n_pix + 63u) / 64u, n_chunks = cpf * job.n_frames;
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < n_chunks; c += n_waves) {
        const uint32_t fr = __builtin_amdgcn_readfirstlane(c / cpf);
        const uint32_t pix = (c - fr * cpf) * 64u + (threadIdx.x & 63u);
        if (pix < n_pix) aov_pixel(sc, q, job, fr, pix, n_pix, err);
    }
}
#endif

uint64_t aov_max_items() { return (uint64_t)0x7FFFFFFFu * kAovThreads; }

// The built policies (mm_variants.h) as one table: per policy the two kernels' instances.
constexpr int kAovKeys[] = {
#define MM_AOV(P) (P),
    MM_AOV_POLICIES(MM_AOV)
#undef MM_AOV
};
constexpr size_t kAovCount = sizeof(kAovKeys) / sizeof(kAovKeys[0]);
struct AovTable {
    void (*query[kAovCount])(DevScene, const float4*, uint64_t, RayHit*, uint32_t*);
    void (*aov[kAovCount])(DevScene, AovJob, uint32_t*);
};
template <size_t... I>
static AovTable aov_table(std::index_sequence<I...>) {
    return {{k_query_rays<kAovKeys[I]>...}, {k_trace_aov<kAovKeys[I]>...}};
}
static const AovTable kAovTable = aov_table(std::make_index_sequence<kAovCount>{});

// The table's row, or kAovCount when the policy is not built.
static size_t find_variant(int policy) {
    size_t i = 0;
    while (i < kAovCount && kAovKeys[i] != policy) ++i;
    return i;
}

hipError_t launch_query_rays(const DevScene& sc, int policy, const float4* rays, uint64_t n_rays, RayHit* hits,
                             uint32_t* err, hipStream_t s) {
    const size_t v = find_variant(policy);
    if (v == kAovCount || n_rays == 0 || n_rays > aov_max_items()) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n_rays + kAovThreads - 1) / kAovThreads));
    hipLaunchKernelGGL(kAovTable.query[v], grid, dim3(kAovThreads), 0, s, sc, rays, n_rays, hits, err);
    return hipGetLastError();
}

hipError_t launch_trace_aov(const DevScene& sc, int policy, const AovJob& job, uint32_t* err, hipStream_t s) {
    const uint64_t n_pix = (uint64_t)job.w * job.h;
    const uint64_t bpf = (n_pix + kAovThreads - 1) / kAovThreads;
    const size_t v = find_variant(policy);
    if (v == kAovCount || n_pix == 0 || n_pix > 0x7FFFFFFFu || job.n_frames == 0 || bpf * job.n_frames > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
#ifdef MM_AOV_AB_LDS
    if (policy == kAovGrid + kAovGridFlat + kAovGridWide && sc.grid.bytes <= 64 * 1024) {
        int dev = 0, cus = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const uint64_t blocks = std::min<uint64_t>(2 * (uint64_t)cus, (n_pix * job.n_frames + 1023) / 1024);
        hipLaunchKernelGGL(k_trace_aov_lds<kAovGrid + kAovGridFlat + kAovGridWide>, dim3((uint32_t)blocks), dim3(1024),
                           sc.grid.bytes, s, sc, job, err);
        return hipGetLastError();
    }
#endif
    const dim3 grid((uint32_t)(bpf * job.n_frames));
    hipLaunchKernelGGL(kAovTable.aov[v], grid, dim3(kAovThreads), 0, s, sc, job, err);
    return hipGetLastError();
}

}  // namespace mm
