// mm_launch.h — host-callable launchers for the kernels in trace_kernels.hip, display.hip, denoise_kernels.hip,
// temporal_kernels.hip and upsample_kernels.hip, and the argument structs they take.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "mm_calls.h"
#include "mm_device.h"

namespace mm {

// Per-rect derived data for the scene (n, |v|, |u|, kind) from raw rects.
hipError_t launch_prep_rects(const mm_rect* rects_dev, uint32_t n, float4* geo_dev, hipStream_t s);

// Parity mode: the reference dispatch (grid_w x grid_h groups of 32x32).
hipError_t launch_trace_chunks(const DevScene& sc, const mm_uniform& u, const uint32_t* chunks_dev,
                               uint32_t grid_w, uint32_t grid_h, float4* fb, uint32_t* fb8,
                               unsigned long long* stats_dev, uint32_t* err, bool count_stats, hipStream_t s);

// A staged sample: the path's value sqrt(max(L, 0)) (shaders.metal:342-344),
// 12 B -- the resolve reads these back (round 6: 16-B float4 slots before, a
// quarter of the staged traffic unused).
using Sample = F3;
static_assert(sizeof(Sample) == 12, "three floats, no padding");

// Deferred path states (mirror-tail deferral): one 64-byte record per entry
// (rec[4*i .. 4*i+3] = ori.xyz dir.x | dir.yz T.xy | T.z L.xyz | sb,
// (n - mh) | mh << 15, sample slot, mask: the trial window -- one base pointer; 16 SoA field arrays would
// hold 15 addresses in SGPRs across the bounce loop), `cap` records; resident
// block b owns the kTailRing records from b * kTailRing (its tail ring, at most
// 2 blocks per CU; kTailRing: mm_variants.h).

struct TailQueue {
    uint4* rec = nullptr;
    uint32_t cap = 0;
};

struct TileJob {
    mm_uniform u;
    mm_ext e;
    uint32_t x0, y0, w, h, y_stride;
    uint32_t view_w;     // (uint32_t)u.view_w — pixel index stride
    // Fused resolve (wave-persistent kernel, 64 % spp == 0): each wave reduces
    // its chunk's whole pixels in registers and writes out[pixel] itself, in
    // k_resolve's order; no per-sample staging buffer, no resolve launch.
    void* out = nullptr;  // float4 per pixel, or RGBA8 (4 B) with MM_EXT_RGBA8 (mm_wave_util.h store_pixel)
    uint32_t fuse = 0;
    // 1: a pixel-list launch (mm_trace_pixels): `pixels` below names the pixels.  (In the padding ahead of
    // wave_ts: every other member keeps the offset it had without it.)
    // 2: the pixel lists of several frames in one launch (mm_trace_pixel_lists): `lists` below is the launch's
    // list table, which names the pixels.
    // 3 (kListRays): a ray-list launch (mm_trace_rays): `rays` below holds the paths' origins, directions and
    // RNG keys; no pixel is named, so the resolves take the tile path (w = n_rays, h = 1).
    uint32_t list = 0;
    // Diagnostics (mm_set_wave_timeline): per wave of the wave-persistent
    // kernel, 4 x u64 = (entry, LDS staged, exit, chunks) in wall_clock64()
    // ticks (100 MHz).  Null = off.
    unsigned long long* wave_ts = nullptr;
    uint32_t wave_ts_cap = 0;
    // Multi-frame launch (mm_trace_tile_frames; wave-persistent kernel, fused
    // resolve): the queue holds n_frames frames' chunks back to back; frame f
    // uses RNG frame e.frame + f and writes out + f * w * h.
    uint32_t n_frames = 1;
    // CUs' worth of blocks the wave-persistent grid leaves free (MM_OPT_RESERVE_CUS)
    uint32_t reserve_cus = 0;
    // Mirror-tail deferral (MM_OPT_DEFER; wave-persistent kernel, samples
    // staged per path, no fused resolve): a wave whose paths are at bounce
    // >= defer_from with at most defer_lanes lanes still running queues those
    // paths' state in its block's tail ring (ballot + prefix compaction, one
    // LDS atomic per wave) and moves on; the block's waves take 64 queued tails
    // at a time as a chunk.  Sample slot of a path: fr * (w*h*spp) + path.
    // defer_from >= 2^30: off.
    uint32_t defer_from = 1u << 30, defer_lanes = 0;
    TailQueue tail;
    // 1: the rings' records in LDS (the kRing = 2 kernel, where the grid image leaves room); 0: in `tail`
    uint32_t ring_lds = 0;
    // Ray list (mm_trace_rays, `list` == kListRays): MM_RAYS_JITTER -- the record's direction gets the primary
    // ray's jitter (the seed's first two draws) before the first bounce.  Launch-uniform; read by the kList == 3
    // instances only.  (In the padding ahead of `status`: every other member keeps its offset.)
    uint32_t ray_jitter = 0;
    // Per-launch status word (host-mapped pinned memory, mm_runtime.hip): the
    // last wave of the launch moves the error flag into it, | kStatusDone, so
    // the host attributes an error to the call that launched it without a
    // sync.  Null: the error flag stays sticky (parity mode reads it itself).
    uint32_t* status = nullptr;
    // Polls a tail-ring protocol wait may take before it gives up (error bit
    // 2; ~50 ms; a wait lasts at most a few bounces).  The round-3 trip of the
    // 64-lane deferral test was a livelock ending at the 32-bit entry
    // counters' wrap, not a slow wait (trace_kernels.hip).
    // MM_OPT_FAULT_INJECT 2 sets 0.
    uint32_t ring_spin = 1u << 20;
    // The launch's first timed-out ring wait writes 16 words here
    // (host-mapped; trace_kernels.hip ring_timeout); launch_id goes into it.
    uint32_t* ring_diag = nullptr;
    uint32_t launch_id = 0;
    // MM_OPT_FAULT_INJECT 1: the launch raises error bit 3; 4: its first
    // deferred path is lost (bit 4, and the reader's ring timeout) -- tests of
    // the error path.
    uint32_t fault = 0;
    // Trials of the rejection sampling a new-path chunk draws into each path's
    // window before its bounces (MM_OPT_PREDRAW, mm_plan.cpp; 0..31; mm_trace.h
    // predraw_trials).  Results never depend on it.
    uint32_t predraw = 0;
    // Pooled top-up rounds after them (MM_OPT_PREDRAW_POOL; mm_trace.h pool_trials): the accepted trials a
    // path's window should hold before its bounces, min(bounce_limit - 1, 31); 0: none.
    uint32_t predraw_pool = 0;
    // Camera sequence (mm_trace_tile_cameras): frame f of the launch is traced with camera record f of this
    // device array (kCamStride floats per record: an mm_camera, padded to 64 B) instead of u.cam.  Null:
    // u.cam for every frame.  (Last member: the offsets of the fields above are those of the launches
    // without it.)
    //
    // Pixel list (mm_trace_pixels, `list` set): the launch is w = n_pixels, h = 1, one camera, one frame, and
    // entry e's pixel is record e of the device array `pixels`, (x, y) in view coordinates, instead of
    // (x0 + i, y0 + j * y_stride); an entry outside the view is not traced (mm_wave_util.h list_pixel).  Read by
    // the kList instances only.  A launch has cameras or a list, never both, and the two pointers share the
    // slot: a member more would move the kernel arguments behind the job, and the camera-sequence instances'
    // register allocation with them (profiles/pixels/kernel_resources.txt).
    //
    // Pixel lists of several frames (mm_trace_pixel_lists, `list` == 2): the slot points at the launch's list
    // table (ListTable below) -- the pixel array's address travels in its header, so the job needs no second
    // pointer.  w = the entries of all lists together, h = 1; read by the kList == 2 instances only.
    //
    // Ray list (mm_trace_rays, `list` == kListRays): the launch is w = n_rays, h = 1, one frame, no camera, and
    // entry e's path starts from record e of the device array `rays`, two float4: (ox, oy, oz, key) and
    // (dx, dy, dz, -), mm_query_rays' record with the RNG key's bits in word 3.  Every entry is traced.  Read by
    // the kList == 3 instances only.
    union {
        const float* cams = nullptr;
        const uint2* pixels;
        const uint32_t* lists;
        const float4* rays;
    };
};
constexpr uint32_t kListRays = 3;
static_assert(sizeof(TileJob) == 224, "the kernel-argument layout the tile instances were measured with");
constexpr uint32_t kCamStride = 16;
static_assert(sizeof(mm_camera) <= kCamStride * sizeof(float), "a camera record holds an mm_camera");

// The list table of an mm_trace_pixel_lists launch, an array of 32-bit words in device memory (written by a
// copy that precedes the launch on its stream, by nothing while it runs; the kernel reads it with scalar loads):
//   words 0..7                   header: the pixel array's address (low, high), n_lists, the queue's chunks, the
//                                word offset of the records, 3 unused
//   words 8..8 + n_lists         first chunk of every list, non-decreasing, and the queue's chunks once more:
//                                chunk c belongs to the LAST list f with first[f] <= c (an empty list shares
//                                its value with its successor; trailing empty lists hold the queue's chunks)
//   words rec .. rec + 16 n      one 16-word record per list: the camera (10 floats), the RNG frame, the first
//                                chunk, the chunks, the first global entry, the paths (entries * spp), the entries
// rec is a multiple of 16 words, and so is the table's address: a record is one aligned 64-byte line.
namespace ListTable {
constexpr uint32_t kPixLo = 0, kPixHi = 1, kLists = 2, kChunks = 3, kRecords = 4, kHeader = 8, kRecWords = 16;
constexpr uint32_t kKey = 10, kFirstChunk = 11, kNumChunks = 12, kFirstEntry = 13, kPaths = 14, kEntries = 15;
constexpr uint32_t records_at(uint32_t n_lists) { return (kHeader + n_lists + 1u + 15u) & ~15u; }
constexpr size_t words(uint32_t n_lists) { return (size_t)records_at(n_lists) + (size_t)kRecWords * n_lists; }
}  // namespace ListTable
static_assert(sizeof(mm_camera) <= ListTable::kKey * sizeof(float), "a list record's camera words hold an mm_camera");

// (Error flag bits kErr* and kStatusDone: mm_calls.h.)
// One-thread kernel that publishes a non-persistent launch's error flag into
// its status word (the persistent kernel's last wave does this itself).
hipError_t launch_publish_status(uint32_t* err, uint32_t* status, hipStream_t s);

struct MegaOpts {
    bool reference = false;   // traverse_reference (IEEE division): MM_PIPE_REFERENCE, the only form built
    uint32_t block = 256;     // threads per workgroup
};

// MM_PIPE_REFERENCE: one thread per (pixel, sample) path; writes
// the per-sample value sqrt(max(L,0)) to samples[path] (path = pixel*spp+s).
hipError_t launch_trace_mega(const DevScene& sc, const TileJob& job, Sample* samples,
                             unsigned long long* stats_dev, uint32_t* err, bool count_stats,
                             const MegaOpts& o, hipStream_t s);

// Throughput mode, wave-persistent megakernel: resident 1024-thread blocks,
// waves pull 64-path chunks from work[0]; work[0..1] must be zero at launch
// and are left zero by the kernel itself (the last wave re-zeroes them).
// lds_mode / form: trace_kernels.hip (k_trace_wavepersist); returns
// hipErrorInvalidValue for a pair that is not instantiated.
hipError_t launch_trace_wavepersist(const DevScene& sc, const TileJob& job, Sample* samples,
                                    unsigned long long* stats, uint32_t* err, uint32_t* work, bool count_stats,
                                    int lds_mode, int form, hipStream_t s);
size_t wavepersist_lds_bytes(const DevScene& sc, int lds_mode);
// (wavepersist_grid_cap, wavepersist_defer_built, wavepersist_built: mm_variants.h)
// Register / scratch / LDS use of the (kStats = false) instance.
// ring: 0 no tail deferral, 1 rings with global records, 2 rings with records in LDS.
hipError_t wavepersist_attributes(int lds_mode, int form, int ring, hipFuncAttributes* a);
// Display stage (display.hip).
hipError_t launch_present_blur(const uint32_t* in, uint32_t* out, uint32_t W, uint32_t H, hipStream_t s);
hipError_t launch_chunk_packets(const float4* fb, const uint32_t* chunks, uint32_t n_chunks, uint32_t W, uint32_t H,
                                float4* out, hipStream_t s);
hipError_t launch_quantize(const float4* in, uint32_t* out, size_t n, hipStream_t s);

// One pass of mm_denoise_frames over one frame (denoise_kernels.hip); every pointer points at that frame.
struct DnPass {
    const float4* in = nullptr;      // the pass's input image
    const float4* nd = nullptr;      // guide: normal_depth
    const uint2* keys = nullptr;     // guide: the packed (id, bits of albedo.w) records of launch_denoise_keys
    void* out = nullptr;             // float4 per pixel, or RGBA8 (4 B) when rgba8 is set
    uint32_t w = 0, h = 0, tiles_x = 0;  // w * h < 2^31; tiles_x: set by the launcher
    uint32_t s = 1;                  // tap spacing, 1 << pass
    float sigma_z = 0.0f, sigma_l = 0.0f, sl = 0.0f;  // sl = sigma_l * (1.0f / (float)s)
    uint32_t rgba8 = 0;
};
hipError_t launch_denoise_keys(const float4* al, const uint32_t* id, uint2* keys, size_t n, hipStream_t s);
hipError_t launch_denoise_pass(const DnPass& pass, hipStream_t s);

// One pass of mm_denoise_frames_var over one frame (denoise_kernels.hip, the kVar instances); every pointer points
// at that frame.  The members it shares with DnPass have DnPass's names (the pass templates take either), and the
// layout is the one its instances were measured with.
struct DnVarPass {
    const float4* in = nullptr;      // the pass's input image
    const float* vin = nullptr;      // the pass's input variance (of the pixel mean's luminance)
    const float4* nd = nullptr;      // guide: normal_depth
    const uint2* keys = nullptr;     // guide: the packed (id, bits of albedo.w) records of launch_denoise_keys
    void* out = nullptr;             // float4 per pixel, or RGBA8 (4 B) when rgba8 is set
    float* vout = nullptr;           // the pass's output variance; nullptr: not stored
    uint32_t w = 0, h = 0, tiles_x = 0;  // w * h < 2^31; tiles_x: set by the launcher
    uint32_t s = 1;                  // tap spacing, 1 << pass
    float sigma_z = 0.0f, sigma_l = 0.0f, eps_l = 0.0f;  // the stop: sigma_l * sqrt(3x3 mean of vin) + eps_l
    uint32_t rgba8 = 0;
};
hipError_t launch_denoise_var_pass(const DnVarPass& pass, hipStream_t s);

// One frame of mm_accumulate_frames (temporal_kernels.hip); every pointer points at one frame.
struct TpFrame {
    const float4* color = nullptr;   // the frame as traced
    const float4* nd = nullptr;      // its guides
    const float4* al = nullptr;
    const uint32_t* id = nullptr;
    const float4* h_color = nullptr; // the history frame's output (alpha = N); nullptr: no history frame
    const float4* h_nd = nullptr;    // its guides
    const float4* h_al = nullptr;
    const uint32_t* h_id = nullptr;
    float4* out = nullptr;
    mm_camera cam{}, h_cam{};        // the frame's and the history frame's camera
    float view_w = 0.0f, view_h = 0.0f;
    uint32_t x0 = 0, y0 = 0, w = 0, h = 0;  // w * h < 2^31; x0 + w, y0 + h <= 2^24
    uint32_t tiles_x = 0;                   // set by the launcher
    float n_max = 1.0f, tol_z = 0.0f, w_min = 0.0f;      // n_max as a float (exact: at most 65535)
};
hipError_t launch_temporal_frame(const TpFrame& frame, hipStream_t s);

// mm_blend_pixels (temporal_kernels.hip): n list entries' extra samples into the accumulated window.
struct TpBlend {
    float4* image = nullptr;         // the window's w * h pixels (alpha = N), updated in place
    const uint2* pixels = nullptr;   // n entries (x, y), view coordinates
    const float4* extra = nullptr;   // n entries: the extra samples' mean (an mm_trace_pixels output)
    uint64_t n = 0;                  // (n + 255) / 256 < 2^31
    uint32_t x0 = 0, y0 = 0, w = 0, h = 0;  // w * h < 2^31
    float m = 0.0f;                  // weight of the extra samples, in frames
};
hipError_t launch_blend_pixels(const TpBlend& blend, hipStream_t s);

// One frame of mm_accumulate_frames_var (temporal_kernels.hip, kVar): TpFrame, and the variances beside it.
struct TpFrameVar {
    TpFrame f;                       // as for mm_accumulate_frames
    const float* vmean = nullptr;    // the frame's variance of the pixel mean's luminance
    const float* weight = nullptr;   // the frame's weight per pixel, in frames; nullptr: 1 everywhere (own kernel)
    const float* h_var = nullptr;    // the history frame's variance output; set whenever f.h_color is
    float* vout = nullptr;
};
hipError_t launch_temporal_frame_var(const TpFrameVar& frame, hipStream_t s);

// mm_blend_pixels_var (temporal_kernels.hip, kVar): TpBlend, and the variance image beside it.
struct TpBlendVar {
    TpBlend b;                          // as for mm_blend_pixels
    float* var = nullptr;               // the window's w * h variances, updated in place
    const float* extra_vmean = nullptr; // n entries: the variance of the extra samples' mean
};
hipError_t launch_blend_pixels_var(const TpBlendVar& blend, hipStream_t s);

// mm_upsample_frames (upsample_kernels.hip): all frames of one call.  Frame f's full-resolution buffers start at
// element f * w * h, its lattice buffers at f * lw * lh.
struct UpFrames {
    const float4* low = nullptr;     // the lattice's traced colours
    const float* vlow = nullptr;     // the lattice's variances of the pixel mean; read only with vout
    const float4* nd = nullptr;      // full-resolution guides
    const float4* al = nullptr;
    const uint32_t* id = nullptr;
    float4* out = nullptr;
    float* wout = nullptr;           // nullptr: no weight output (own kernel)
    float* vout = nullptr;           // nullptr: no variance output (own kernel); set only with vlow
    uint32_t w = 0, h = 0, lw = 0, lh = 0;  // w * h < 2^31; lw = ceil(w / scale), lh = ceil(h / scale)
    uint32_t n_frames = 0;
    uint32_t shift = 1;              // log2(scale): 1, 2 or 3
    uint32_t tiles_x = 0, tiles = 0; // set by the launcher: 64 x 4 tiles per row / per frame
    float inv_s = 0.5f;              // 1.0f / (float)scale (exact)
    float w_min = 0.0f;
    bool lds = true;                 // MM_OPT_UPSAMPLE_LDS: stage the block's lattice footprint in LDS (else: gathers)
};
// (hipErrorInvalidValue for more blocks than one launch holds: check_upsample's bound, mm_filter_args.h)
hipError_t launch_upsample_frames(const UpFrames& frames, hipStream_t s);

// mm_fill_pixels (upsample_kernels.hip): n list entries replace their pixels of the window's images.
struct UpFill {
    float4* image = nullptr;         // the window's w * h pixels
    float* var = nullptr;            // its variances; nullptr: none (then extra_vmean is nullptr too)
    float* weight = nullptr;         // its weights; nullptr: none
    const uint2* pixels = nullptr;   // n entries (x, y), view coordinates
    const float4* extra = nullptr;   // n entries: the traced pixels
    const float* extra_vmean = nullptr;
    uint64_t n = 0;                  // (n + 255) / 256 < 2^31
    uint32_t x0 = 0, y0 = 0, w = 0, h = 0;  // w * h < 2^31
    float m = 0.0f;                  // what weight[p] becomes
};
hipError_t launch_fill_pixels(const UpFill& fill, hipStream_t s);

// Per-pixel reduction of spp samples in the reference's order, then / spp.
hipError_t launch_resolve(const TileJob& job, const Sample* samples, void* out, hipStream_t s);
// The same pixel, and the unbiased sample variance of the samples' luminance into var[pixel] (spp >= 2;
// mm_trace_tile_var / mm_trace_pixels_var, include/mm_api.h).  var travels beside the job, as out does:
// TileJob keeps the layout the trace kernels were measured with.
hipError_t launch_resolve_var(const TileJob& job, const Sample* samples, void* out, float* var, hipStream_t s);

}  // namespace mm
