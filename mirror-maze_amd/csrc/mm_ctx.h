// mm_ctx.h — the context behind the C ABI's opaque mm_ctx (include/mm_api.h),
// shared by the runtime (mm_runtime.hip), the trace and query calls
// (mm_trace_calls.hip), the frame filters' calls (mm_filters.hip) and the
// multi-GPU frame path (mm_comm.hip), with the four files' error plumbing
// (fail, HIPC, ensure) and the runtime's helpers the trace calls share.
// Private to the library.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mm_api.h"
#include "mm_calls.h"
#include "mm_launch.h"
#include "mm_stage_ring.h"

using mm::DevGrid;

constexpr uint32_t kStatusSlots = 1024;

struct mm_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // scene (buffers 1,2,3,5,6 of compute_shader)
    mm_rect* d_rects = nullptr;
    float4* d_nodes = nullptr;      // production layout (packed child words)
    float4* d_nodes_ref = nullptr;  // reference layout
    uint32_t root_packed = 0;
    bool fast_ok = false;
    uint32_t depth = 0;         // tree depth = max traversal stack entries
    float4* d_geo = nullptr;
    float4* d_shade = nullptr;
    uint2* d_recs = nullptr;    // compact leaf-ordered rect records
    size_t n_fast_recs = 0;
    bool lean_ok = false;       // no SLOW rect records (loop form 7, grid search)
    uint8_t* d_grid = nullptr;  // certified grid search (grid_build.cpp, mm_grid.h)
    DevGrid grid{};
    bool grid_ok = false;
    bool grid_slow = false;  // the grid has SLOW records (general rect test)
    bool grid_wide = false;  // 64-bit cell words with per-face list ranges
    bool grid_flat = false;  // the flat forms apply (grid_build.h GridHost::flat_ok)
    uint32_t grid_classes = 0;  // threshold classes of its compact records (GridHost::n_class; MM_INFO_GRID_CLASSES)
    std::string grid_why;
    uint32_t* d_idx = nullptr;
    uint32_t n_rects = 0, n_nodes = 0;
    bool has_scene = false;
    // texout (parity mode)
    float4* d_fb = nullptr;
    uint32_t* d_fb8 = nullptr;
    uint32_t* d_fb8_alt = nullptr;  // presentation blur target (swapped with d_fb8)
    uint32_t last_chunks = 0;       // chunk count of the last mm_trace_chunks
    float4* d_packets = nullptr;
    size_t packets_cap = 0;
    uint32_t fb_w = 0, fb_h = 0;
    // chunk list (buffer 0)
    uint32_t* d_chunks = nullptr;
    size_t chunks_cap = 0;
    // per-sample staging (throughput mode)
    mm::Sample* d_samples = nullptr;
    size_t samples_cap = 0;
    // mirror-tail rings' records (MM_OPT_DEFER)
    void* d_tail = nullptr;
    uint32_t tail_cap = 0;
    // the staging rings (mm_stage_ring.h; mm_trace_calls.hip stage): the camera records of mm_trace_tile_cameras
    // and mm_trace_aov launches (mm::kCamStride floats each; at least 8 records, wrapping from 4096 on), and the
    // list tables of mm_trace_pixel_lists launches (mm_launch.h ListTable; at least 1024 words, wrapping from
    // 2^22 on).  Two rings: a table never waits for camera records' launches, nor the other way round.
    mm::StageRing cams{8 * mm::kCamStride, 4096 * mm::kCamStride};
    mm::StageRing lists{1024, 1u << 22};
    // mm_denoise_frames' scratch (mm_filters.hip dn_begin): the two intermediate images a frame's passes alternate between (one frame
    // each, `dn_img_cap` pixels in all) and the call's packed key records (`dn_keys_cap`).  A call's kernels are
    // ordered after the last call's on the same stream; `dn_done` (recorded after every call) orders them when
    // the stream changed.  mm_denoise_frames_var shares all of it, under the same bookkeeping, and keeps the
    // variance images between its passes beside it (`d_dn_var`: one frame of floats per ping-pong side).
    float4* d_dn_img = nullptr;
    size_t dn_img_cap = 0;
    float* d_dn_var = nullptr;
    size_t dn_var_cap = 0;
    uint2* d_dn_keys = nullptr;
    size_t dn_keys_cap = 0;
    hipEvent_t dn_done = nullptr;
    hipStream_t dn_stream = nullptr;
    bool dn_pending = false;
    // aux: stats[4] (u64) + error flag (u32)
    unsigned long long* d_aux = nullptr;
    uint32_t* d_work = nullptr;  // the wave-persistent kernel's self-cleaning queue heads + waves-done word (4 KB)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // The last call that used the state a context's launches share -- d_work, d_aux, d_samples, d_tail, the
    // status slots, the parity-mode buffers: its work is done at `shared_done`, recorded on `shared_stream`.  A
    // later such call on another stream waits for that event first (mm_runtime.hip order_shared), as the denoise
    // calls do for their scratch (dn_done).  The event is the `ev1` end_timing records after a call's last
    // launch anyway, so a trace call pays nothing for it; mm_present, which is not timed, records
    // `present_done`.
    hipEvent_t shared_done = nullptr;
    hipStream_t shared_stream = nullptr;
    hipEvent_t present_done = nullptr;
    float last_ms = 0.0f;
    uint32_t last_launches = 0;
    int pipe = MM_PIPE_AUTO;
    // options (include/mm_api.h MM_OPT_*); defaults = the measured fastest
    bool opt_lds = true;            // stage scene data in LDS where it fits
    uint32_t opt_block = 0;         // k_trace_mega block size (0 = auto)
    int opt_persist = 2;            // 0 one thread per path (k_trace_mega), 2 wave-persistent
    int opt_ww = -1;                // loop form: -1 auto, 0, 5, 7 (BVH), 11 (grid search)
    int opt_lds_rects = 1;          // compact rect records in LDS beside the nodes when they fit
    bool opt_fuse = true;           // resolve fused into the wave when 64 % spp == 0
    uint32_t opt_reserve_cus = 0;   // MM_OPT_RESERVE_CUS
    int opt_defer = -1;             // MM_OPT_DEFER: defer a wave's paths once <= this many lanes run (0 off, -1 auto)
    uint32_t opt_defer_min = 1u << 24;  // MM_OPT_DEFER_MIN: ... in launches of at least this many paths
    int last_form = -1, last_mode = -1;  // of the last wave-persistent launch (mm_scene_info)
    unsigned long long* d_wave_ts = nullptr;  // diagnostics (mm_set_wave_timeline)
    uint32_t wave_ts_cap = 0;
    // per-kernel profiling of the trace kernel (mm_set_profiling)
    bool prof = false;
    std::vector<hipEvent_t> prof_ev;   // pairs (start, stop)
    size_t prof_used = 0;              // events recorded since last reset
    // Per-launch status words (host-mapped pinned memory, kStatusSlots + kRingDiagWords of them) and the
    // numbered calls that own them: mm_calls.h.
    uint32_t* h_status = nullptr;
    uint32_t* d_status = nullptr;
    mm::CallTracker calls;
    int opt_predraw = -1;        // MM_OPT_PREDRAW: trials pre-drawn per path at a chunk's start (-1: by the bounce limit)
    bool opt_predraw_pool = true;  // MM_OPT_PREDRAW_POOL: pooled top-up rounds after the pre-pass's own rounds
    bool opt_upsample_lds = true;  // MM_OPT_UPSAMPLE_LDS: mm_upsample_frames stages its lattice footprint in LDS
    int opt_fault = 0;           // MM_OPT_FAULT_INJECT
    bool opt_grid_merge = true;  // MM_OPT_GRID_MERGE (read by mm_upload_scene)
    int opt_grid_cell = 100;     // MM_OPT_GRID_CELL (read by mm_upload_scene)
    bool opt_grid_wide = true;   // MM_OPT_GRID_WIDE (read by mm_upload_scene)
    bool last_defer = false;     // the last trace call ran the tail rings
    int last_kern_mode = -1, last_kern_form = -1;  // for MM_INFO_LAST_VGPRS / _SCRATCH
    int last_kern_ring = 0;      // its tail-ring kind (wavepersist_attributes: 0 none, 1 global, 2 LDS records)
    // frame-end gather (mm_comm.hip): the root's receive staging, one slab per rank
    uint8_t* d_gather = nullptr;
    size_t gather_cap = 0;
    // the last gather that used d_gather: its assembly is done at this event (recorded on the stream the gather
    // ran on); a gather on another stream waits for it before reusing the staging, and a regrow waits before
    // freeing it (two gathers on different streams raced on the one staging buffer)
    hipEvent_t gather_done = nullptr;
    bool gather_pending = false;
};

namespace mm {
// Record `msg` as the context's last error and return `code`.
inline int ctx_fail(mm_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
inline int fail(mm_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }

// Return MM_ERR_HIP from the calling function, with the runtime's message, if a HIP call fails.
#define HIPC(ctx, expr)                                                                               \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return mm::ctx_fail((ctx), MM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// A device array of at least `n` elements: kept if it is large enough, else freed and allocated anew.
template <typename T>
int ensure(mm_ctx* c, T*& ptr, size_t& cap, size_t n) {
    if (n <= cap && ptr) return MM_OK;
    if (ptr) { (void)hipFree(ptr); ptr = nullptr; cap = 0; }
    HIPC(c, hipMalloc((void**)&ptr, std::max<size_t>(n, 1) * sizeof(T)));
    cap = n;
    return MM_OK;
}

// ensure for scratch that queued launches may still read, on any stream used so far: grown (never shrunk) after
// everything the device has queued is done.  The wait costs something only when growing.
template <typename T>
int ensure_idle(mm_ctx* c, T*& ptr, size_t& cap, size_t n) {
    if (n <= cap && ptr) return MM_OK;
    HIPC(c, hipDeviceSynchronize());
    return ensure(c, ptr, cap, n);
}

// The runtime's helpers the trace and query calls use too (mm_runtime.hip).
DevScene dev_scene(const mm_ctx* c);
// Before a call's first use of the state the context's launches share: if the last such call was enqueued on
// another stream, the context's stream waits for its end (an event wait on the device; the host never waits).
int order_shared(mm_ctx* c);
// The events around a call's launches (mm_last_timing).  end_timing's event is also what order_shared waits for.
int begin_timing(mm_ctx* c);
int end_timing(mm_ctx* c, uint32_t launches);
// Reads the statistics (st, if not null) and the sticky error flag back, after a sync of the stream.
int read_aux(mm_ctx* c, mm_stats* st);
// An earlier call that failed on the GPU is reported first, by name (mm_calls.h).
int report_failure(mm_ctx* c, const char* suffix);
}  // namespace mm
