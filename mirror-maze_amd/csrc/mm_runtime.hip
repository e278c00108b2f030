// mm_runtime.hip — the C ABI of include/mm_api.h over the HIP runtime (the
// frame filters' six calls: mm_filters.hip; the multi-GPU path: mm_comm.hip).
//
// Replaces the reference's Metal plumbing: device/queue creation
// (src/main.rs:616-626), buffer creation and updates (src/utils.rs:86-102,
// src/main.rs:723-730, 784) and the compute dispatch (src/main.rs:867-886).
// No exception or abort crosses the ABI; every HIP error becomes
// MM_ERR_HIP with the runtime's message in mm_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "grid_build.h"
#include "mm_aov.h"
#include "mm_api.h"
#include "mm_ctx.h"
#include "mm_filter_args.h"
#include "mm_launch.h"
#include "mm_plan.h"

using namespace mm;

namespace mm {
size_t build_compact_rects(const mm_rect* rects, uint32_t n_rects, const uint32_t* idx, std::vector<uint32_t>& out,
                           size_t* n_slow);
}

constexpr uint32_t kStatusSlots = 1024;

namespace {

DevScene dev_scene(const mm_ctx* c) {
    DevScene s;
    s.nodes = c->d_nodes;
    s.nodes_ref = c->d_nodes_ref;
    s.root_packed = c->root_packed;
    s.fast_ok = c->fast_ok ? 1u : 0u;
    s.geo = c->d_geo;
    s.recs = c->d_recs;
    s.grid = c->grid;
    s.shade = c->d_shade;
    s.idx = c->d_idx;
    s.n_nodes = c->n_nodes;
    s.n_rects = c->n_rects;
    return s;
}

// The policy's inputs (mm_plan.h) from the context.
SceneFacts scene_facts(const mm_ctx* c) {
    SceneFacts f;
    f.grid_ok = c->grid_ok; f.grid_slow = c->grid_slow; f.grid_wide = c->grid_wide; f.grid_flat = c->grid_flat;
    f.lean_ok = c->lean_ok;
    f.n_nodes = c->n_nodes; f.n_rects = c->n_rects;
    f.bytes = c->grid.bytes; f.off_box = c->grid.off_box; f.off_data = c->grid.off_data;
    f.grid_why = c->grid_why.c_str();
    return f;
}
PlanOptions plan_options(const mm_ctx* c) {
    PlanOptions o;
    o.pipe = c->pipe; o.opt_ww = c->opt_ww; o.opt_lds = c->opt_lds; o.opt_lds_rects = c->opt_lds_rects;
    o.opt_fuse = c->opt_fuse; o.opt_persist = c->opt_persist; o.opt_defer = c->opt_defer;
    o.opt_defer_min = c->opt_defer_min;
    o.opt_predraw = c->opt_predraw;
    o.opt_predraw_pool = c->opt_predraw_pool;
    return o;
}

void free_scene(mm_ctx* c) {
    (void)hipFree(c->d_rects); (void)hipFree(c->d_nodes); (void)hipFree(c->d_nodes_ref); (void)hipFree(c->d_geo);
    (void)hipFree(c->d_shade); (void)hipFree(c->d_idx); (void)hipFree(c->d_recs);
    (void)hipFree(c->d_grid);
    c->d_grid = nullptr; c->grid = DevGrid{}; c->grid_ok = false; c->grid_slow = false; c->grid_wide = false;
    c->grid_flat = false; c->grid_classes = 0;
    c->d_rects = nullptr; c->d_nodes = nullptr; c->d_nodes_ref = nullptr; c->d_geo = nullptr; c->d_recs = nullptr; c->d_shade = nullptr; c->d_idx = nullptr;
    c->has_scene = false;
}

// Stack depth the near-first traversal can reach: at most one pending far
// child per level, so the tree depth bounds it.
int check_tree(const mm_node* nodes, uint32_t n_nodes, const uint32_t* idx, uint32_t n_rects, std::string& why,
               uint32_t* depth_out) {
    for (uint32_t i = 0; i < n_rects; ++i)
        if (idx[i] >= n_rects) { why = "idx out of range"; return MM_ERR_INVALID; }
    std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, 0u}};
    std::vector<uint8_t> seen(n_nodes, 0);
    uint32_t maxd = 0;
    while (!todo.empty()) {
        auto [n, d] = todo.back();
        todo.pop_back();
        if (n >= n_nodes || seen[n]) { why = "node graph is not a tree"; return MM_ERR_INVALID; }
        seen[n] = 1;
        maxd = std::max(maxd, d);
        const mm_node& nd = nodes[n];
        if (nd.count > 0) {
            if ((uint64_t)nd.left_first + nd.count > n_rects) { why = "leaf range out of bounds"; return MM_ERR_INVALID; }
        } else {
            if ((uint64_t)nd.left_first + 1 >= n_nodes) { why = "child index out of range"; return MM_ERR_INVALID; }
            todo.push_back({nd.left_first, d + 1});
            todo.push_back({nd.left_first + 1, d + 1});
        }
    }
    if (maxd > (uint32_t)kStackMax) { why = "BVH deeper than the 50-entry traversal stack"; return MM_ERR_STACK; }
    *depth_out = maxd;
    return MM_OK;
}

// Coordinates inside the Markstein-quotient guard (mm_trace.h): 0 or
// |x| in [2^-30, 2^60]; rect extents 0 or |x| in [2^-10, 2^60].
bool coord_ok(float x) {
    const float a = std::fabs(x);
    return a == 0.0f || (a >= 0x1p-30f && a <= 0x1p60f);
}
bool extent_ok(float x) {
    const float a = std::fabs(x);
    return a == 0.0f || (a >= 0x1p-10f && a <= 0x1p60f);
}

// The tail rings' records (mm_launch.h TailQueue): kTailRing per resident
// block, at most 2 blocks per CU.
int tail_queue(mm_ctx* c, TailQueue& q) {
    int cus = 0;
    HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const uint32_t cap = 2u * (uint32_t)cus * kTailRing;
    if (c->tail_cap < cap || !c->d_tail) {
        (void)hipFree(c->d_tail);
        c->d_tail = nullptr;
        c->tail_cap = 0;
        HIPC(c, hipMalloc(&c->d_tail, (size_t)cap * 64));
        c->tail_cap = cap;
    }
    q.rec = reinterpret_cast<uint4*>(c->d_tail);
    q.cap = c->tail_cap;
    return MM_OK;
}

// The device records of a camera-sequence launch (mm_launch.h TileJob::cams): the caller's cameras go into a
// pinned staging ring (consumed when this returns) and from there to the ring's device mirror by a copy on
// the context's stream, ahead of the launch that reads them.  Every call takes fresh records, so a later
// call's cameras never land on those of a launch still running, and nothing here waits for the GPU -- except
// when the ring is full: then everything the device has queued is waited for once, and the ring grows (up to
// kCamsWrap records, from where on it wraps instead).
constexpr size_t kCamsMin = 8, kCamsWrap = 4096;
int stage_cameras(mm_ctx* c, const mm_camera* cams, uint32_t n, const float*& dev) {
    if (c->cams_next + n > c->cams_cap) {
        HIPC(c, hipDeviceSynchronize());  // staged records may still be on their way, on any stream used so far
        if (n > c->cams_cap || c->cams_cap < kCamsWrap) {
            const size_t cap = std::max<size_t>({kCamsMin, 2 * c->cams_cap, n});
            if (c->h_cams) (void)hipHostFree(c->h_cams);
            (void)hipFree(c->d_cams);
            c->h_cams = nullptr; c->d_cams = nullptr; c->cams_cap = 0;
            HIPC(c, hipHostMalloc((void**)&c->h_cams, cap * kCamStride * sizeof(float), hipHostMallocDefault));
            HIPC(c, hipMalloc((void**)&c->d_cams, cap * kCamStride * sizeof(float)));
            c->cams_cap = cap;
        }
        c->cams_next = 0;
    }
    float* h = c->h_cams + c->cams_next * kCamStride;
    std::memset(h, 0, (size_t)n * kCamStride * sizeof(float));
    for (uint32_t f = 0; f < n; ++f) std::memcpy(h + (size_t)f * kCamStride, &cams[f], sizeof(mm_camera));
    float* d = c->d_cams + c->cams_next * kCamStride;
    HIPC(c, hipMemcpyAsync(d, h, (size_t)n * kCamStride * sizeof(float), hipMemcpyHostToDevice, c->stream));
    c->cams_next += n;
    dev = d;
    return MM_OK;
}

// The list table of an mm_trace_pixel_lists launch (mm_launch.h ListTable), staged as stage_cameras stages
// camera records: `words` words (a multiple of 16, so every table starts on a 64-byte line) of a pinned ring
// that `fill` writes, mirrored to the device by a copy on the context's stream ahead of the launch.  Every
// call takes fresh words; nothing waits for the GPU unless the ring is full (then once, and the ring grows up
// to kListsWrap words, from where on it wraps).
constexpr size_t kListsMin = 1024, kListsWrap = 1u << 22;
template <typename F>
int stage_lists(mm_ctx* c, size_t words, F&& fill, const uint32_t*& dev) {
    if (c->lists_next + words > c->lists_cap) {
        HIPC(c, hipDeviceSynchronize());  // staged tables may still be on their way, on any stream used so far
        if (words > c->lists_cap || c->lists_cap < kListsWrap) {
            const size_t cap = std::max<size_t>({kListsMin, 2 * c->lists_cap, words});
            if (c->h_lists) (void)hipHostFree(c->h_lists);
            (void)hipFree(c->d_lists);
            c->h_lists = nullptr; c->d_lists = nullptr; c->lists_cap = 0;
            HIPC(c, hipHostMalloc((void**)&c->h_lists, cap * sizeof(uint32_t), hipHostMallocDefault));
            HIPC(c, hipMalloc((void**)&c->d_lists, cap * sizeof(uint32_t)));
            c->lists_cap = cap;
        }
        c->lists_next = 0;
    }
    uint32_t* h = c->h_lists + c->lists_next;
    std::memset(h, 0, words * sizeof(uint32_t));
    fill(h);
    uint32_t* d = c->d_lists + c->lists_next;
    HIPC(c, hipMemcpyAsync(d, h, words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    c->lists_next += words;
    dev = d;
    return MM_OK;
}

int begin_timing(mm_ctx* c) {
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    return MM_OK;
}
int end_timing(mm_ctx* c, uint32_t launches) {
    HIPC(c, hipEventRecord(c->ev1, c->stream));
    c->last_launches = launches;
    c->last_ms = -1.0f;  // resolved lazily in mm_last_timing
    return MM_OK;
}

// Bracket one trace-kernel launch with events when profiling is on.
int prof_mark(mm_ctx* c) {
    if (!c->prof) return MM_OK;
    if (c->prof_used == c->prof_ev.size()) {
        hipEvent_t e;
        HIPC(c, hipEventCreate(&e));
        c->prof_ev.push_back(e);
    }
    HIPC(c, hipEventRecord(c->prof_ev[c->prof_used++], c->stream));
    return MM_OK;
}

int read_aux(mm_ctx* c, mm_stats* st) {
    unsigned long long h[5];
    HIPC(c, hipMemcpyAsync(h, c->d_aux, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (st) { st->rays = h[0]; st->node_visits = h[1]; st->rect_tests = h[2]; st->paths = h[3]; }
    if ((uint32_t)h[4] != 0) {
        HIPC(c, hipMemsetAsync(c->d_aux + 4, 0, sizeof(unsigned long long), c->stream));
        if (h[4] & 2u) return fail(c, MM_ERR_HIP, "tail ring wait timed out (kernel protocol error)");
        return fail(c, MM_ERR_STACK, "traversal stack overflow (depth > 50)");
    }
    return MM_OK;
}

// ---- per-call status (mm_calls.h) -------------------------------------------
// An earlier call that failed on the GPU is reported first, by name.
int report_failure(mm_ctx* c, const char* suffix) { return c->calls.report_failure(suffix, c->err); }

// One launch of the open call (CallTracker::begin_call): takes its status slot, runs
// launch(status word, launch id) -- which enqueues the kernel and returns MM_OK or what fail() gave it --
// and, unless the kernel publishes its status itself (self_publish: the wave-persistent kernel's last wave
// does), enqueues the publish of the error flag into the status word.  The slot is taken first (its device
// address is a kernel argument); if the launch then fails to enqueue, the slot is released as
// finished-clean, and the call is still tracked for the launches it did enqueue.
template <typename L>
int enqueue_launch(mm_ctx* c, bool self_publish, L&& launch) {
    uint32_t slot = 0;
    if (int rc = c->calls.next_status(slot, c->err)) return rc;
    int rc = prof_mark(c);
    if (!rc) rc = launch(c->d_status + slot, (uint32_t)c->calls.last_launch());
    if (rc) {
        c->calls.release_unqueued();
        return rc;
    }
    if (!self_publish) {
        uint32_t* err_dev = reinterpret_cast<uint32_t*>(c->d_aux + 4);
        const hipError_t pe = launch_publish_status(err_dev, c->d_status + slot, c->stream);
        if (pe != hipSuccess) {
            // fold the kernel's error flag into THIS launch's slot (after a sync), so it is
            // never published by -- and blamed on -- a later call's launch
            uint32_t bits = 0;
            (void)hipStreamSynchronize(c->stream);
            (void)hipMemcpy(&bits, err_dev, sizeof(bits), hipMemcpyDeviceToHost);
            (void)hipMemset(err_dev, 0, sizeof(bits));
            c->calls.fold_unpublished(bits);
            return fail(c, MM_ERR_HIP, std::string("launch_publish_status: ") + hipGetErrorString(pe));
        }
    }
    return prof_mark(c);
}

// The view and tile checks shared by the trace calls; `name` prefixes the messages.  e: the sampling
// parameters of a call that has them (mm_trace_tile*), else null and the call's own mirror limit.
int check_tile(mm_ctx* c, const char* name, const mm_uniform* u, const mm_ext* e, uint32_t mirror_limit, uint32_t x0,
               uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride) {
    auto bad = [&](const char* what) { return fail(c, MM_ERR_INVALID, std::string(name) + ": " + what); };
    if (!(u->view_w >= 1.0f && u->view_w <= 65536.0f && u->view_h >= 1.0f && u->view_h <= 65536.0f))
        return bad("bad view size");
    const uint32_t W = (uint32_t)u->view_w, H = (uint32_t)u->view_h;
    if (w == 0 || h == 0 || y_stride == 0 || (e && (e->spp == 0 || e->spp > 4096)))
        return bad(e ? "empty tile or bad spp" : "empty tile");
    // the tail records pack bounces | mirror hits << 16 (trace_kernels.hip tail_store)
    if ((e && e->bounce_limit > 32767) || mirror_limit > 32767)
        return bad(e ? "bounce or mirror limit above 32767" : "mirror limit above 32767");
    if ((uint64_t)x0 + w > W || (uint64_t)y0 + (uint64_t)(h - 1) * y_stride >= H) return bad("tile outside the frame");
    return MM_OK;
}

}  // namespace

extern "C" {

const char* mm_version(void) {
    return "mirror-maze-amd 0.4 gfx950";
}

int mm_create(int device, mm_ctx** out) {
    if (!out) return MM_ERR_INVALID;
    *out = nullptr;
    mm_ctx* c = new (std::nothrow) mm_ctx();
    if (!c) return MM_ERR_NOMEM;
    c->device = device;
    int rc = MM_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == MM_OK) rc = fail(c, MM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    int n = 0;
    chk(hipGetDeviceCount(&n), "hipGetDeviceCount");
    if (rc == MM_OK && (device < 0 || device >= n)) rc = fail(c, MM_ERR_INVALID, "no such HIP device");
    if (rc == MM_OK) chk(hipSetDevice(device), "hipSetDevice");
    if (rc == MM_OK) chk(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking), "hipStreamCreate");
    if (rc == MM_OK) chk(hipEventCreate(&c->ev0), "hipEventCreate");
    if (rc == MM_OK) chk(hipEventCreate(&c->ev1), "hipEventCreate");
    if (rc == MM_OK) chk(hipMalloc((void**)&c->d_aux, 8 * sizeof(unsigned long long)), "hipMalloc(aux)");
    if (rc == MM_OK) chk(hipMemset(c->d_aux, 0, 8 * sizeof(unsigned long long)), "hipMemset(aux)");
    if (rc == MM_OK) chk(hipMalloc((void**)&c->d_work, 4096), "hipMalloc(work)");
    if (rc == MM_OK) chk(hipMemset(c->d_work, 0, 4096), "hipMemset(work)");
    if (rc == MM_OK)
        chk(hipHostMalloc((void**)&c->h_status, (kStatusSlots + kRingDiagWords) * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocCoherent),
            "hipHostMalloc(status)");
    if (rc == MM_OK) chk(hipHostGetDevicePointer((void**)&c->d_status, c->h_status, 0), "hipHostGetDevicePointer");
    if (rc == MM_OK)  // (the tracker waits for a status slot's earlier launch: the stream, then the device)
        c->calls = CallTracker(c->h_status, [c](int level) -> int {
            if (level == 0) HIPC(c, hipStreamSynchronize(c->stream));
            else HIPC(c, hipDeviceSynchronize());
            return MM_OK;
        }, kStatusSlots);
    if (rc != MM_OK) {
        fprintf(stderr, "mm_create: %s\n", c->err.c_str());
        mm_destroy(c);
        return rc;
    }
    c->stream = c->own_stream;
    *out = c;
    return MM_OK;
}

void mm_destroy(mm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_scene(c);
    (void)hipFree(c->d_fb); (void)hipFree(c->d_fb8); (void)hipFree(c->d_chunks);
    (void)hipFree(c->d_fb8_alt); (void)hipFree(c->d_packets);
    (void)hipFree(c->d_samples); (void)hipFree(c->d_aux); (void)hipFree(c->d_tail); (void)hipFree(c->d_work);
    (void)hipFree(c->d_gather);
    (void)hipFree(c->d_cams);
    if (c->h_cams) (void)hipHostFree(c->h_cams);
    (void)hipFree(c->d_lists);
    if (c->h_lists) (void)hipHostFree(c->h_lists);
    (void)hipFree(c->d_dn_img); (void)hipFree(c->d_dn_keys); (void)hipFree(c->d_dn_var);
    if (c->dn_done) (void)hipEventDestroy(c->dn_done);
    if (c->gather_done) (void)hipEventDestroy(c->gather_done);
    if (c->h_status) (void)hipHostFree(c->h_status);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* mm_last_error(const mm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int mm_set_stream(mm_ctx* c, void* s) {
    if (!c) return MM_ERR_INVALID;
    c->stream = (s == MM_OWN_STREAM) ? c->own_stream : (hipStream_t)s;
    return MM_OK;
}

int mm_set_wave_timeline(mm_ctx* c, unsigned long long* buf, uint32_t n_waves) {
    if (!c) return MM_ERR_INVALID;
    c->d_wave_ts = n_waves ? buf : nullptr;
    c->wave_ts_cap = buf ? n_waves : 0;
    return MM_OK;
}

int mm_get_stream(const mm_ctx* c, void** s) {
    if (!c || !s) return MM_ERR_INVALID;
    *s = (void*)c->stream;
    return MM_OK;
}

int mm_set_pipeline(mm_ctx* c, int pipe) {
    if (!c) return MM_ERR_INVALID;
    if (pipe < MM_PIPE_AUTO || pipe > MM_PIPE_REFERENCE) return fail(c, MM_ERR_INVALID, "unknown pipeline");
    c->pipe = pipe;
    return MM_OK;
}

// Kernel variants removed in round 6: every one measured slower than what
// MM_PIPE_AUTO selects; the options that chose them are refused by name.
static const char* const kRemoved =
    "this kernel variant (one thread per path over the production BVH forms, loop form 0, the split node "
    "cache, dictionary-coded nodes) measured slower and was removed (DESIGN.md §4)";

int mm_set_option(mm_ctx* c, int key, int value) {
    if (!c) return MM_ERR_INVALID;
    switch (key) {
        case MM_OPT_LDS_NODES: c->opt_lds = value != 0; return MM_OK;
        case MM_OPT_BLOCK:
            if (value < 64 || value > 1024 || value % 64) return fail(c, MM_ERR_INVALID, "block must be 64..1024, x64");
            c->opt_block = (uint32_t)value;
            return MM_OK;
        case MM_OPT_PERSIST:
            if (value != 0 && value != 2) return fail(c, MM_ERR_INVALID, "persist must be 0 or 2");
            if (value == 0) return fail(c, MM_ERR_UNSUPPORTED, kRemoved);
            c->opt_persist = value;
            return MM_OK;
        case MM_OPT_TRAVERSAL:
            if (value != -1 && value != 0 && value != 5 && value != 7 && value != 11)
                return fail(c, MM_ERR_INVALID, "traversal must be -1 (auto), 0, 5, 7 or 11 (grid search)");
            if (value == 0) return fail(c, MM_ERR_UNSUPPORTED, kRemoved);
            c->opt_ww = value;
            return MM_OK;
        case MM_OPT_LDS_RECTS: c->opt_lds_rects = value != 0; return MM_OK;
        case MM_OPT_LDS_SPLIT:
            if (value < 0) return fail(c, MM_ERR_INVALID, "split cache size must be >= 0 (0 off, 1 auto, else KB)");
            if (value > 1) return fail(c, MM_ERR_UNSUPPORTED, kRemoved);
            return MM_OK;  // 0 / 1: accepted, nothing to select (no split cache is built)
        case MM_OPT_FUSE_RESOLVE: c->opt_fuse = value != 0; return MM_OK;
        case MM_OPT_RESERVE_CUS:
            if (value < 0 || value > 128) return fail(c, MM_ERR_INVALID, "reserved CUs must be 0..128");
            c->opt_reserve_cus = (uint32_t)value;
            return MM_OK;
        case MM_OPT_DEFER:
            if (value < 0 || value > 64) return fail(c, MM_ERR_INVALID, "defer lanes must be 0..64");
            c->opt_defer = value;
            return MM_OK;
        case MM_OPT_DEFER_MIN:
            if (value < 0) return fail(c, MM_ERR_INVALID, "defer min paths must be >= 0");
            c->opt_defer_min = (uint32_t)value;
            return MM_OK;
        case MM_OPT_DICT_NODES:
            if (value < 0 || value > 2) return fail(c, MM_ERR_INVALID, "dict nodes must be 0, 1 or 2");
            if (value == 2) return fail(c, MM_ERR_UNSUPPORTED, kRemoved);
            return MM_OK;  // 0 / 1: accepted, nothing to select (no dictionary is built)
        case MM_OPT_GRID_MERGE: c->opt_grid_merge = value != 0; return MM_OK;
        case MM_OPT_GRID_WIDE: c->opt_grid_wide = value != 0; return MM_OK;
        case MM_OPT_GRID_CELL:
            if (value < 25 || value > 400) return fail(c, MM_ERR_INVALID, "grid cell scale must be 25..400 (%)");
            c->opt_grid_cell = value;
            return MM_OK;
        case MM_OPT_PREDRAW:
            if (value < -1 || value > 31) return fail(c, MM_ERR_INVALID, "pre-drawn trials must be -1 (auto) or 0..31");
            c->opt_predraw = value;
            return MM_OK;
        case MM_OPT_PREDRAW_POOL:
            if (value < 0 || value > 1) return fail(c, MM_ERR_INVALID, "pre-pass pooling must be 0 or 1");
            c->opt_predraw_pool = value != 0;
            return MM_OK;
        case MM_OPT_FAULT_INJECT:
            if (value < 0 || value > 4) return fail(c, MM_ERR_INVALID, "fault inject must be 0..4");
            c->opt_fault = value;
            return MM_OK;
        default: return fail(c, MM_ERR_INVALID, "unknown option");
    }
}

int mm_scene_info(const mm_ctx* c, int key, double* value) {
    if (!c || !value) return MM_ERR_INVALID;
    if (!c->has_scene) return MM_ERR_NO_SCENE;
    const DevGrid& g = c->grid;
    switch (key) {
        case MM_INFO_GRID_OK: *value = c->grid_ok ? 1.0 : 0.0; return MM_OK;
        case MM_INFO_GRID_CELLS_X: *value = g.n[0]; return MM_OK;
        case MM_INFO_GRID_CELLS_Y: *value = g.n[1]; return MM_OK;
        case MM_INFO_GRID_CELLS_Z: *value = g.n[2]; return MM_OK;
        case MM_INFO_GRID_GLOBAL: *value = g.n_glob; return MM_OK;
        case MM_INFO_GRID_BYTES: *value = g.bytes; return MM_OK;
        case MM_INFO_GRID_INDEX_BYTES: *value = g.off_data; return MM_OK;
        case MM_INFO_LEAN: *value = c->lean_ok ? 1.0 : 0.0; return MM_OK;
        case MM_INFO_DEPTH: *value = c->depth; return MM_OK;
        case MM_INFO_DICT_OK: *value = 0.0; return MM_OK;  // (dictionary-coded nodes removed in round 6)
        case MM_INFO_LAST_FORM: *value = c->last_form; return MM_OK;
        case MM_INFO_LAST_LDS_MODE: *value = c->last_mode; return MM_OK;
        case MM_INFO_GRID_FACES: *value = c->grid_ok && c->grid_wide ? 1.0 : 0.0; return MM_OK;
        case MM_INFO_LAST_DEFER: *value = c->last_defer ? 1.0 : 0.0; return MM_OK;
        case MM_INFO_GRID_LDS_CAP: *value = wavepersist_grid_cap(0); return MM_OK;
        case MM_INFO_GRID_FLAT: *value = c->grid_ok && c->grid_flat ? 1.0 : 0.0; return MM_OK;
        case MM_INFO_GRID_SLAB: *value = c->grid_ok && g.slab && g.slab_y[0] < g.slab_y[1] ? 1.0 : 0.0; return MM_OK;
        case MM_INFO_GRID_CLASSES: *value = c->grid_ok ? c->grid_classes : 0u; return MM_OK;
        case MM_INFO_LAST_VGPRS:
        case MM_INFO_LAST_SCRATCH:
        case MM_INFO_LAST_STATIC_LDS: {
            if (c->last_kern_mode < 0) return MM_ERR_INVALID;
            hipFuncAttributes a{};
            if (wavepersist_attributes(c->last_kern_mode, c->last_kern_form, c->last_kern_ring, &a) != hipSuccess)
                return MM_ERR_HIP;
            *value = key == MM_INFO_LAST_VGPRS ? a.numRegs
                     : key == MM_INFO_LAST_SCRATCH ? (double)a.localSizeBytes : (double)a.sharedSizeBytes;
            return MM_OK;
        }
        default: return MM_ERR_INVALID;
    }
}

int mm_upload_scene(mm_ctx* c, const mm_rect* rects, uint32_t n_rects, const mm_node* nodes, uint32_t n_nodes,
                    const uint32_t* idx, const uint8_t* is_mirror, const float* emission) {
    if (!c) return MM_ERR_INVALID;
    if (!rects || !nodes || !idx || !is_mirror || !emission || n_rects == 0 || n_nodes == 0)
        return fail(c, MM_ERR_INVALID, "mm_upload_scene: null array or empty scene");
    if (n_nodes > 2 * n_rects) return fail(c, MM_ERR_INVALID, "mm_upload_scene: more than 2n-1 nodes");
    std::string why;
    uint32_t depth = 0;
    int rc = check_tree(nodes, n_nodes, idx, n_rects, why, &depth);
    if (rc != MM_OK) return fail(c, rc, "mm_upload_scene: " + why);
    // Production node layout: a = (mn.x, mx.x, mn.y, mx.y), b = (mn.z, mx.z, packed, 0),
    // packed = count << 24 | left_first.  Child pairs are renumbered
    // breadth-first from the root's pair, which lands at node 2 (nodes 0-1 are
    // never read: the root is not tested, shaders.metal:123-125), so every pair
    // is one aligned 64-B line and a prefix of the array is the top of the tree
    // (the split LDS cache of mm_trace.h).  Only traversal order matters to the
    // result, and it depends on distances, not on indices.
    for (uint32_t i = 0; i < n_nodes; ++i)
        if (nodes[i].count >= 256u || nodes[i].left_first >= (1u << 24))
            return fail(c, MM_ERR_UNSUPPORTED, "mm_upload_scene: leaf with >= 256 planes or index >= 2^24");
    std::vector<uint32_t> pair_old;  // old index of each pair's left node, breadth-first
    if (nodes[0].count == 0) pair_old.push_back(nodes[0].left_first);
    for (size_t q = 0; q < pair_old.size(); ++q)
        for (uint32_t k = 0; k < 2; ++k) {
            const mm_node& nd = nodes[pair_old[q] + k];
            if (nd.count == 0) pair_old.push_back(nd.left_first);
        }
    std::vector<uint32_t> pair_new(n_nodes, 0);  // old left index -> new left index
    for (size_t q = 0; q < pair_old.size(); ++q) pair_new[pair_old[q]] = 2 + 2 * (uint32_t)q;
    if (2 + 2 * pair_old.size() >= (1u << 24))
        return fail(c, MM_ERR_UNSUPPORTED, "mm_upload_scene: node index >= 2^24");
    auto pack = [&](const mm_node& nd) {
        return nd.count > 0 ? (nd.count << 24) | nd.left_first : pair_new[nd.left_first];
    };
    const uint32_t n_prod = 2 + 2 * (uint32_t)pair_old.size();
    std::vector<float4> packed(2 * (size_t)n_prod, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t q = 0; q < pair_old.size(); ++q)
        for (uint32_t k = 0; k < 2; ++k) {
            const mm_node& nd = nodes[pair_old[q] + k];
            const uint32_t pk = pack(nd);
            float pkf;
            std::memcpy(&pkf, &pk, 4);
            const size_t i = 2 + 2 * q + k;
            packed[2 * i] = make_float4(nd.mn[0], nd.mx[0], nd.mn[1], nd.mx[1]);
            packed[2 * i + 1] = make_float4(nd.mn[2], nd.mx[2], pkf, 0.0f);
        }
    bool fast = true;
    for (uint32_t i = 0; i < n_nodes && fast; ++i)
        for (int a = 0; a < 3; ++a) fast = fast && coord_ok(nodes[i].mn[a]) && coord_ok(nodes[i].mx[a]);
    for (uint32_t k = 0; k < n_rects && fast; ++k)
        for (int a = 0; a < 3; ++a)
            fast = fast && coord_ok(rects[k].o[a]) && extent_ok(rects[k].v[a]) && extent_ok(rects[k].u[a]);
    HIPC(c, hipSetDevice(c->device));
    free_scene(c);
    std::vector<float4> shade(2 * (size_t)n_rects);
    for (uint32_t k = 0; k < n_rects; ++k) {
        shade[2 * k] = make_float4(rects[k].color[0], rects[k].color[1], rects[k].color[2], is_mirror[k] ? 1.0f : 0.0f);
        shade[2 * k + 1] = make_float4(emission[4 * k], emission[4 * k + 1], emission[4 * k + 2], emission[4 * k + 3]);
    }
    HIPC(c, hipMalloc((void**)&c->d_rects, n_rects * sizeof(mm_rect)));
    HIPC(c, hipMalloc((void**)&c->d_nodes, packed.size() * sizeof(float4)));
    HIPC(c, hipMalloc((void**)&c->d_nodes_ref, n_nodes * sizeof(mm_node)));
    HIPC(c, hipMalloc((void**)&c->d_geo, 4 * (size_t)n_rects * sizeof(float4)));
    HIPC(c, hipMalloc((void**)&c->d_shade, 2 * (size_t)n_rects * sizeof(float4)));
    HIPC(c, hipMalloc((void**)&c->d_idx, n_rects * sizeof(uint32_t)));
    std::vector<uint32_t> recs;
    size_t n_slow = n_rects;
    c->n_fast_recs = n_rects < (1u << 20) ? build_compact_rects(rects, n_rects, idx, recs, &n_slow) : 0;
    if (n_rects >= (1u << 20)) recs.assign(10 * (size_t)n_rects, 2u << 30);  // all SLOW (index does not fit)
    HIPC(c, hipMalloc((void**)&c->d_recs, recs.size() * sizeof(uint32_t)));
    HIPC(c, hipMemcpyAsync(c->d_recs, recs.data(), recs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_rects, rects, n_rects * sizeof(mm_rect), hipMemcpyHostToDevice, c->stream));
    // mm_node is exactly two float4: (mn.xyz, mx.x) (mx.yz, left_first, count)
    HIPC(c, hipMemcpyAsync(c->d_nodes_ref, nodes, n_nodes * sizeof(mm_node), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_nodes, packed.data(), packed.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    // certified grid search (mm_grid.h): needs the Markstein guards and axis-aligned rects
    GridHost gh;
    std::string gwhy;
    // the budget: what the static grid array of modes 11 / 14 holds beside the kernel's other static LDS
    // (wavepersist_grid_cap(0), 80 KB -- the LDS of one of the two 1024-thread blocks per CU -- less its
    // claimed-range words; ADVICE r05: an image between that and 80 KB failed the launch)
    const bool grid_ok = fast && build_grid(rects, n_rects, nodes, n_nodes, idx, wavepersist_grid_cap(0), gh, gwhy,
                                            c->opt_grid_merge, c->opt_grid_cell / 100.0, c->opt_grid_wide);
    if (!fast) gwhy = "scene coordinates outside the exact-division guards";
    DevGrid dg{};
    if (grid_ok) {
        // the image, then the leaf boxes (cold: only the full certificate reads them, mm_grid.h)
        const size_t box_bytes = gh.boxes.size() * sizeof(float);
        HIPC(c, hipMalloc((void**)&c->d_grid, gh.bytes + box_bytes));
        HIPC(c, hipMemcpyAsync(c->d_grid, gh.image.data(), gh.bytes, hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(c->d_grid + gh.bytes, gh.boxes.data(), box_bytes, hipMemcpyHostToDevice, c->stream));
        dg = dev_grid(gh, c->d_grid);
        c->grid_slow = gh.n_slow > 0;
        c->grid_wide = gh.wide;
        c->grid_flat = gh.flat_ok;
        c->grid_classes = gh.n_class;
    }
    HIPC(c, hipMemcpyAsync(c->d_shade, shade.data(), shade.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(c->d_idx, idx, n_rects * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(c, launch_prep_rects(c->d_rects, n_rects, c->d_geo, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));  // host arrays may be freed on return
    c->n_rects = n_rects;
    c->n_nodes = n_prod;
    c->root_packed = pack(nodes[0]);
    c->depth = depth;
    c->fast_ok = fast;
    c->lean_ok = n_slow == 0;
    c->grid = dg;
    c->grid_ok = grid_ok;
    c->grid_why = grid_ok ? std::string() : gwhy;
    c->has_scene = true;
    return MM_OK;
}

int mm_trace_chunks(mm_ctx* c, const mm_uniform* u, const uint32_t* chunks, uint32_t n_chunks) {
    if (!c) return MM_ERR_INVALID;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_trace_chunks: no scene uploaded");
    if (!u || !chunks) return fail(c, MM_ERR_INVALID, "mm_trace_chunks: null argument");
    if (!(u->view_w >= 1.0f && u->view_w <= 65536.0f && u->view_h >= 1.0f && u->view_h <= 65536.0f))
        return fail(c, MM_ERR_INVALID, "mm_trace_chunks: bad view size");
    // The kernel maps one wave64 to one pixel's samples: 32x32 threads / ppc
    // must be 64, i.e. chunk_w = 4 as in the reference (main.rs:602).
    if (u->chunk_w != 4) return fail(c, MM_ERR_UNSUPPORTED, "mm_trace_chunks: chunk_w must be 4 (64 samples/pixel)");
    const uint32_t ppc = 16;
    const uint32_t gw = (uint32_t)(u->view_w / 2.0f / (float)ppc), gh = (uint32_t)(u->view_h / 2.0f / (float)ppc);
    if (gw == 0 || gh == 0) return fail(c, MM_ERR_INVALID, "mm_trace_chunks: view too small for one group");
    // every pixel_buffer_index the groups compute (in float, IR %26-%31) must be in range
    uint32_t max_pbi = 0;
    for (uint32_t gy = 0; gy < gh; ++gy) {
        float f = ((u->view_w * 0.5f) * (float)gy) / (float)ppc + (float)(gw - 1);
        max_pbi = std::max(max_pbi, (uint32_t)f);
    }
    if (max_pbi >= n_chunks) return fail(c, MM_ERR_INVALID, "mm_trace_chunks: chunk list shorter than the grid");
    const uint32_t W = (uint32_t)u->view_w, H = (uint32_t)u->view_h;
    HIPC(c, hipSetDevice(c->device));
    if (W != c->fb_w || H != c->fb_h) {
        (void)hipFree(c->d_fb); (void)hipFree(c->d_fb8); (void)hipFree(c->d_fb8_alt);
        c->d_fb = nullptr; c->d_fb8 = nullptr; c->d_fb8_alt = nullptr;
        c->fb_w = c->fb_h = 0;
        HIPC(c, hipMalloc((void**)&c->d_fb, (size_t)W * H * sizeof(float4)));
        HIPC(c, hipMalloc((void**)&c->d_fb8, (size_t)W * H * sizeof(uint32_t)));
        HIPC(c, hipMalloc((void**)&c->d_fb8_alt, (size_t)W * H * sizeof(uint32_t)));
        HIPC(c, hipMemsetAsync(c->d_fb, 0, (size_t)W * H * sizeof(float4), c->stream));
        HIPC(c, hipMemsetAsync(c->d_fb8, 0, (size_t)W * H * sizeof(uint32_t), c->stream));
        c->fb_w = W; c->fb_h = H;
    }
    int rc = ensure(c, c->d_chunks, c->chunks_cap, 2 * (size_t)n_chunks);
    if (rc) return rc;
    HIPC(c, hipMemcpyAsync(c->d_chunks, chunks, 2 * (size_t)n_chunks * sizeof(uint32_t), hipMemcpyHostToDevice,
                           c->stream));
    HIPC(c, hipMemsetAsync(c->d_aux, 0, 5 * sizeof(unsigned long long), c->stream));  // stats, error flag
    if ((rc = begin_timing(c))) return rc;
    HIPC(c, launch_trace_chunks(dev_scene(c), *u, c->d_chunks, gw, gh, c->d_fb, c->d_fb8, c->d_aux,
                                reinterpret_cast<uint32_t*>(c->d_aux + 4), false, c->stream));
    if ((rc = end_timing(c, 1))) return rc;
    c->last_chunks = n_chunks;
    return read_aux(c, nullptr);
}

int mm_present(mm_ctx* c) {
    if (!c) return MM_ERR_INVALID;
    if (!c->d_fb8) return fail(c, MM_ERR_INVALID, "mm_present: nothing rendered yet");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, launch_present_blur(c->d_fb8, c->d_fb8_alt, c->fb_w, c->fb_h, c->stream));
    std::swap(c->d_fb8, c->d_fb8_alt);
    return MM_OK;
}

int mm_read_packets(mm_ctx* c, float* packets, uint32_t n_chunks) {
    if (!c) return MM_ERR_INVALID;
    if (!packets) return fail(c, MM_ERR_INVALID, "mm_read_packets: null output");
    if (!c->d_fb || c->last_chunks == 0) return fail(c, MM_ERR_INVALID, "mm_read_packets: no mm_trace_chunks yet");
    if (n_chunks > c->last_chunks)
        return fail(c, MM_ERR_INVALID, "mm_read_packets: more chunks than the last dispatch used");
    if (n_chunks == 0) return MM_OK;
    HIPC(c, hipSetDevice(c->device));
    int rc = ensure(c, c->d_packets, c->packets_cap, 16 * (size_t)n_chunks);
    if (rc) return rc;
    HIPC(c, launch_chunk_packets(c->d_fb, c->d_chunks, n_chunks, c->fb_w, c->fb_h, c->d_packets, c->stream));
    HIPC(c, hipMemcpyAsync(packets, c->d_packets, 16 * (size_t)n_chunks * sizeof(float4), hipMemcpyDeviceToHost,
                           c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

int mm_quantize_rgba8(mm_ctx* c, const float* rgba_dev, uint8_t* rgba8_dev, uint64_t n_pixels) {
    if (!c) return MM_ERR_INVALID;
    if ((!rgba_dev || !rgba8_dev) && n_pixels) return fail(c, MM_ERR_INVALID, "mm_quantize_rgba8: null buffer");
    if (n_pixels == 0) return MM_OK;
    if (reinterpret_cast<uintptr_t>(rgba_dev) % 16 || reinterpret_cast<uintptr_t>(rgba8_dev) % 4)
        return fail(c, MM_ERR_INVALID, "mm_quantize_rgba8: misaligned buffer");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, launch_quantize(reinterpret_cast<const float4*>(rgba_dev), reinterpret_cast<uint32_t*>(rgba8_dev),
                            (size_t)n_pixels, c->stream));
    return MM_OK;
}

int mm_read_framebuffer(mm_ctx* c, float* rgba, uint8_t* rgba8) {
    if (!c) return MM_ERR_INVALID;
    if (!c->d_fb) return fail(c, MM_ERR_INVALID, "mm_read_framebuffer: nothing rendered yet");
    const size_t n = (size_t)c->fb_w * c->fb_h;
    HIPC(c, hipSetDevice(c->device));
    if (rgba) HIPC(c, hipMemcpyAsync(rgba, c->d_fb, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (rgba8) HIPC(c, hipMemcpyAsync(rgba8, c->d_fb8, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

namespace {

// The additional conditions of the variance calls (name: mm_trace_tile_var / mm_trace_pixels_var): at least
// two samples, no accumulation, and a variance buffer of n floats apart from the output's out_bytes.
int check_var(mm_ctx* c, const char* name, const mm_ext* e, const void* out_dev, uint64_t out_bytes,
              const float* var_dev, uint64_t n) {
    auto bad = [&](const char* what) { return fail(c, MM_ERR_INVALID, std::string(name) + ": " + what); };
    if (e->spp < 2) return bad("a sample variance needs spp >= 2");
    if (e->flags & MM_EXT_ACCUMULATE) return bad("MM_EXT_ACCUMULATE is not supported");
    if (!var_dev) return bad("null var_dev");
    if (reinterpret_cast<uintptr_t>(var_dev) % 4) return bad("var_dev not 4-byte aligned");
    if (ranges_overlap(out_dev, out_bytes, var_dev, n * 4)) return bad("var_dev overlaps out_dev");
    return MM_OK;
}

// cams: null, or the n_frames cameras of a camera-sequence launch (mm_trace_tile_cameras; u->cam is then unused)
// var_call: mm_trace_tile_var -- the samples are staged whatever MM_OPT_FUSE_RESOLVE says, and the resolve
// writes the per-pixel variance to var_dev beside the pixel
int trace_tile_impl(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const mm_ext* e, uint32_t n_frames,
                    uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, void* out_dev,
                    mm_stats* stats, bool var_call = false, float* var_dev = nullptr) {
    if (!c) return MM_ERR_INVALID;
    // the multi-frame entry point this call came through (its conditions apply to a one-camera sequence too)
    const bool multi = n_frames > 1 || cams;
    const char* fn = cams ? "mm_trace_tile_cameras" : "mm_trace_tile_frames";
    // an earlier call that failed on the GPU is reported first, by name; this call is then not enqueued
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_trace_tile: no scene uploaded");
    if (!u || !e || !out_dev) return fail(c, MM_ERR_INVALID, "mm_trace_tile: null argument");
    if (int rc0 = check_tile(c, "mm_trace_tile", u, e, e->mirror_limit, x0, y0, w, h, y_stride)) return rc0;
    if (n_frames == 0) return fail(c, MM_ERR_INVALID, std::string(fn) + ": no frames");
    // MM_EXT_RGBA8: 4-byte RGBA8 pixels (the fused texture-write conversion) instead of float4
    const bool rgba8 = (e->flags & MM_EXT_RGBA8) != 0;
    if (rgba8 && (e->flags & MM_EXT_ACCUMULATE))
        return fail(c, MM_ERR_INVALID, "mm_trace_tile: MM_EXT_RGBA8 frames cannot accumulate");
    const size_t out_bpp = rgba8 ? 4 : 16;
    // the stores are out_bpp wide (a float4 per pixel, or one RGBA8 word): the output must be aligned to that
    if (reinterpret_cast<uintptr_t>(out_dev) % out_bpp)
        return fail(c, MM_ERR_INVALID, std::string("mm_trace_tile: output not ") + std::to_string(out_bpp) +
                                           "-byte aligned");
    if (var_call) {
        // (elements in all, capped where the plan refuses the launch anyway: the byte counts fit 64 bits)
        const uint64_t n_all = std::min<uint64_t>((uint64_t)w * h, (1ull << 40) / n_frames) * n_frames;
        if (int rc0 = check_var(c, "mm_trace_tile_var", e, out_dev, n_all * out_bpp, var_dev, n_all)) return rc0;
    }
    HIPC(c, hipSetDevice(c->device));
    const bool want_stats = (e->flags & MM_EXT_COUNT_STATS) != 0;
    const bool persist = c->pipe != MM_PIPE_REFERENCE && (c->pipe == MM_PIPE_WAVEFRONT || c->opt_persist == 2);
    if (!persist && c->pipe != MM_PIPE_REFERENCE) return fail(c, MM_ERR_UNSUPPORTED, kRemoved);
    // the plan (mm_plan.h): query method and LDS placement, then deferral / ring kind / fused resolve / rows
    // per launch, given the static LDS of the placement's deferral kernels
    const SceneFacts facts = scene_facts(c);
    PlanOptions opts = plan_options(c);
    if (var_call) opts.opt_fuse = false;  // the variance is taken of the staged samples
    int form = 0, mode = 0;
    if (persist) {
        Choice m = choose_method(facts, opts);
        if (m.code == MM_OK) m = choose_placement(facts, opts, m.form);
        if (m.code != MM_OK) return fail(c, m.code, m.error);
        form = m.form;
        mode = m.mode;
    }
    size_t static_lds[2] = {kNotBuilt, kNotBuilt};
    if (persist && wavepersist_defer_built(mode, form) && (c->opt_defer != 0 || c->pipe == MM_PIPE_WAVEFRONT))
        for (int kind : {1, 2}) {
            hipFuncAttributes a{};
            // (a static-grid placement is fitted to the array's capacity: the kernel's own figure is not read)
            if (lds_static_grid(mode)) static_lds[kind - 1] = 0;
            else if (wavepersist_attributes(mode, form, kind, &a) == hipSuccess) static_lds[kind - 1] = a.sharedSizeBytes;
        }
    const LaunchPlan plan = plan_tile(facts, opts, form, mode, static_lds, *e, w, h, n_frames, multi ? fn : nullptr);
    if (plan.code != MM_OK) return fail(c, plan.code, plan.error);
    const bool defer = plan.defer, fuse = plan.fuse;
    const uint32_t rows_per_batch = plan.rows_per_batch;
    const uint64_t row_paths = (uint64_t)w * e->spp;
    int rc = fuse ? MM_OK : ensure(c, c->d_samples, c->samples_cap,
                                   (size_t)(row_paths * rows_per_batch) * (defer ? n_frames : 1));
    if (rc) return rc;
    TailQueue tq;
    if (defer && plan.ring == 1 && (rc = tail_queue(c, tq))) return rc;  // (records in LDS: no global ring)
    const float* cams_dev = nullptr;
    if (cams && (rc = stage_cameras(c, cams, n_frames, cams_dev))) return rc;
    // aux: [0..3] stats (zeroed only when counted), [4] error flag (moved into the launch's status word by
    // the launch itself).  d_work: the wave-persistent kernel's queue head(s) and waves-done word
    // (self-cleaning).  No fill kernel on the default path: see k_trace_wavepersist.
    if (want_stats) HIPC(c, hipMemsetAsync(c->d_aux, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = begin_timing(c))) return rc;
    uint32_t* err_dev = reinterpret_cast<uint32_t*>(c->d_aux + 4);
    const DevScene sc = dev_scene(c);
    c->calls.begin_call();
    uint32_t launches = 0;
    for (uint32_t j0 = 0; j0 < h; j0 += rows_per_batch) {
        TileJob job;
        job.u = *u;
        job.e = *e;
        job.x0 = x0;
        job.y0 = y0 + j0 * y_stride;
        job.w = w;
        job.h = std::min(rows_per_batch, h - j0);
        job.y_stride = y_stride;
        job.view_w = (uint32_t)u->view_w;
        job.fuse = fuse ? 1u : 0u;
        job.wave_ts = c->d_wave_ts;
        job.wave_ts_cap = c->wave_ts_cap;
        job.out = reinterpret_cast<char*>(out_dev) + (size_t)j0 * w * out_bpp;
        job.n_frames = n_frames;
        job.cams = cams_dev;
        job.reserve_cus = c->opt_reserve_cus;
        job.predraw = plan.predraw;
        job.predraw_pool = plan.predraw_pool;
        job.fault = (c->opt_fault == 1 || c->opt_fault == 4) ? (uint32_t)c->opt_fault : 0u;
        if (c->opt_fault == 2) job.ring_spin = 0;
        if (defer) {
            job.defer_from = 1;
            job.defer_lanes = c->opt_defer > 0 ? (uint32_t)c->opt_defer : 32u;
            job.tail = tq;
            job.ring_lds = plan.ring == 2 ? 1u : 0u;
        }
        job.ring_diag = c->d_status + kStatusSlots;
        rc = enqueue_launch(c, persist, [&](uint32_t* status, uint32_t launch_id) -> int {
            job.status = status;
            job.launch_id = launch_id;
            if (c->opt_fault == 3) return fail(c, MM_ERR_HIP, "injected enqueue failure (MM_OPT_FAULT_INJECT 3)");
            if (persist) {
                c->last_form = form >= kFormGrid ? kFormGrid : form;
                c->last_mode = mode;
                c->last_kern_mode = mode;
                c->last_kern_form = form;
                c->last_kern_ring = plan.ring;
                HIPC(c, launch_trace_wavepersist(sc, job, c->d_samples, c->d_aux, err_dev,
                                                 c->d_work, want_stats, mode, form,
                                                 c->stream));
            } else {
                MegaOpts mo;
                mo.reference = c->pipe == MM_PIPE_REFERENCE;
                mo.block = c->opt_block ? c->opt_block : 256u;
                HIPC(c, launch_trace_mega(dev_scene(c), job, c->d_samples, c->d_aux, err_dev, want_stats, mo,
                                          c->stream));
            }
            return MM_OK;
        });
        if (rc) break;
        launches += fuse ? 1 : 2;
        if (fuse) continue;
        // the frames' staged samples and output slices are contiguous (a multi-frame launch is one
        // row batch), so one resolve over h x n_frames rows covers them all
        TileJob rj = job;
        if (defer) rj.h = job.h * n_frames;
        // (a later row batch's variances start at its own rows)
        const hipError_t re =
            var_call ? launch_resolve_var(rj, c->d_samples, job.out, var_dev + (size_t)j0 * w, c->stream)
                     : launch_resolve(rj, c->d_samples, job.out, c->stream);
        if (re != hipSuccess) {
            rc = fail(c, MM_ERR_HIP, std::string("launch_resolve: ") + hipGetErrorString(re));
            break;
        }
    }
    c->last_defer = defer;
    char what[160] = "";
    if (c->calls.call_has_launches())  // the launches this call enqueued (all of them unless rc)
        snprintf(what, sizeof(what), "%s, frames %u..%u, tile (%u, %u) %ux%u / %u, %u spp",
                 var_call ? "mm_trace_tile_var" : multi ? fn : "mm_trace_tile", e->frame, e->frame + n_frames - 1, x0,
                 y0, w, h, y_stride, e->spp);
    c->calls.end_call(what);
    if (rc) return rc;
    if ((rc = end_timing(c, launches))) return rc;
    if (want_stats) {
        if ((rc = read_aux(c, stats))) return rc;
        return report_failure(c, "");  // (synced: this call's own error, if any)
    }
    return MM_OK;
}

}  // namespace

int mm_trace_tile(mm_ctx* c, const mm_uniform* u, const mm_ext* e, uint32_t x0, uint32_t y0, uint32_t w,
                  uint32_t h, uint32_t y_stride, float* out_dev, mm_stats* stats) {
    return trace_tile_impl(c, u, nullptr, e, 1, x0, y0, w, h, y_stride, out_dev, stats);
}

int mm_trace_tile_frames(mm_ctx* c, const mm_uniform* u, const mm_ext* e, uint32_t n_frames, uint32_t x0,
                         uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, float* out_dev, mm_stats* stats) {
    return trace_tile_impl(c, u, nullptr, e, n_frames, x0, y0, w, h, y_stride, out_dev, stats);
}

int mm_trace_tile_cameras(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const mm_ext* e, uint32_t n_frames,
                          uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, float* out_dev,
                          mm_stats* stats) {
    if (!c) return MM_ERR_INVALID;
    if (!cams) return fail(c, MM_ERR_INVALID, "mm_trace_tile_cameras: no cameras");
    return trace_tile_impl(c, u, cams, e, n_frames, x0, y0, w, h, y_stride, out_dev, stats);
}

int mm_trace_tile_var(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const mm_ext* e, uint32_t n_frames,
                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, void* out_dev, float* var_dev,
                      mm_stats* stats) {
    return trace_tile_impl(c, u, cams, e, n_frames, x0, y0, w, h, y_stride, out_dev, stats, true, var_dev);
}

namespace {

// var_call: mm_trace_pixels_var, as in trace_tile_impl
int trace_pixels_impl(mm_ctx* c, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels_dev, uint64_t n_pixels,
                      void* out_dev, mm_stats* stats, bool var_call, float* var_dev) {
    if (!c) return MM_ERR_INVALID;
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_trace_pixels: no scene uploaded");
    if (n_pixels == 0) return MM_OK;
    if (!u || !e || !pixels_dev || !out_dev) return fail(c, MM_ERR_INVALID, "mm_trace_pixels: null argument");
    // (the view, spp and the limits: the tile calls' checks, on a one-pixel tile)
    if (int rc0 = check_tile(c, "mm_trace_pixels", u, e, e->mirror_limit, 0, 0, 1, 1, 1)) return rc0;
    const bool rgba8 = (e->flags & MM_EXT_RGBA8) != 0;
    if (rgba8 && (e->flags & MM_EXT_ACCUMULATE))
        return fail(c, MM_ERR_INVALID, "mm_trace_pixels: MM_EXT_RGBA8 results cannot accumulate");
    const size_t out_bpp = rgba8 ? 4 : 16;
    if (reinterpret_cast<uintptr_t>(pixels_dev) % 8 || reinterpret_cast<uintptr_t>(out_dev) % out_bpp)
        return fail(c, MM_ERR_INVALID, std::string("mm_trace_pixels: list not 8-byte or output not ") +
                                           std::to_string(out_bpp) + "-byte aligned");
    if (var_call) {
        if (n_pixels > 0xFFFFFFFFull)  // (the plan's own refusal, ahead of the byte counts below)
            return fail(c, MM_ERR_INVALID, "mm_trace_pixels: more paths than one launch holds (2^32)");
        if (int rc0 = check_var(c, "mm_trace_pixels_var", e, out_dev, n_pixels * out_bpp, var_dev, n_pixels))
            return rc0;
    }
    HIPC(c, hipSetDevice(c->device));
    const bool want_stats = (e->flags & MM_EXT_COUNT_STATS) != 0;
    const bool persist = c->pipe != MM_PIPE_REFERENCE && c->opt_persist == 2;
    const SceneFacts facts = scene_facts(c);
    PlanOptions opts = plan_options(c);
    if (var_call) opts.opt_fuse = false;  // the variance is taken of the staged samples
    // the plan first: its refusals (the queue and staging bounds) need no kernel choice
    const LaunchPlan plan = plan_pixels(opts, *e, n_pixels);
    if (plan.code != MM_OK) return fail(c, plan.code, plan.error);
    int form = 0, mode = 0;
    if (persist) {
        Choice m = choose_method(facts, opts);
        if (m.code == MM_OK) m = choose_placement(facts, opts, m.form);
        if (m.code != MM_OK) return fail(c, m.code, m.error);
        form = m.form;
        mode = m.mode;
    }
    const bool fuse = plan.fuse;
    int rc = fuse ? MM_OK : ensure(c, c->d_samples, c->samples_cap, (size_t)(n_pixels * e->spp));
    if (rc) return rc;
    if (want_stats) HIPC(c, hipMemsetAsync(c->d_aux, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = begin_timing(c))) return rc;
    uint32_t* err_dev = reinterpret_cast<uint32_t*>(c->d_aux + 4);
    const DevScene sc = dev_scene(c);
    // the tile job of a one-row tile n_pixels wide, its pixels named by the list
    TileJob job;
    job.u = *u;
    job.e = *e;
    job.x0 = 0;
    job.y0 = 0;
    job.w = (uint32_t)n_pixels;
    job.h = 1;
    job.y_stride = 1;
    job.view_w = (uint32_t)u->view_w;
    job.fuse = fuse ? 1u : 0u;
    job.wave_ts = c->d_wave_ts;
    job.wave_ts_cap = c->wave_ts_cap;
    job.out = out_dev;
    job.reserve_cus = c->opt_reserve_cus;
    job.predraw = plan.predraw;
    job.predraw_pool = plan.predraw_pool;
    job.fault = c->opt_fault == 1 ? 1u : 0u;
    job.ring_diag = c->d_status + kStatusSlots;
    job.list = 1;
    job.pixels = reinterpret_cast<const uint2*>(pixels_dev);
    c->calls.begin_call();
    rc = enqueue_launch(c, persist, [&](uint32_t* status, uint32_t launch_id) -> int {
        job.status = status;
        job.launch_id = launch_id;
        if (c->opt_fault == 3) return fail(c, MM_ERR_HIP, "injected enqueue failure (MM_OPT_FAULT_INJECT 3)");
        if (persist) {
            c->last_form = form >= kFormGrid ? kFormGrid : form;
            c->last_mode = mode;
            c->last_kern_mode = mode;
            c->last_kern_form = form;
            c->last_kern_ring = 0;
            HIPC(c, launch_trace_wavepersist(sc, job, c->d_samples, c->d_aux, err_dev, c->d_work, want_stats, mode,
                                             form, c->stream));
        } else {
            MegaOpts mo;
            mo.reference = true;
            mo.block = c->opt_block ? c->opt_block : 256u;
            HIPC(c, launch_trace_mega(sc, job, c->d_samples, c->d_aux, err_dev, want_stats, mo, c->stream));
        }
        return MM_OK;
    });
    if (!rc && !fuse) {
        const hipError_t re = var_call ? launch_resolve_var(job, c->d_samples, job.out, var_dev, c->stream)
                                       : launch_resolve(job, c->d_samples, job.out, c->stream);
        if (re != hipSuccess) rc = fail(c, MM_ERR_HIP, std::string("launch_resolve: ") + hipGetErrorString(re));
    }
    c->last_defer = false;
    char what[160] = "";
    if (c->calls.call_has_launches())
        snprintf(what, sizeof(what), "%s, frame %u, %llu pixels, %u spp",
                 var_call ? "mm_trace_pixels_var" : "mm_trace_pixels", e->frame, (unsigned long long)n_pixels, e->spp);
    c->calls.end_call(what);
    if (rc) return rc;
    if ((rc = end_timing(c, fuse ? 1 : 2))) return rc;
    if (want_stats) {
        if ((rc = read_aux(c, stats))) return rc;
        return report_failure(c, "");
    }
    return MM_OK;
}

}  // namespace

int mm_trace_pixels(mm_ctx* c, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels_dev, uint64_t n_pixels,
                    void* out_dev, mm_stats* stats) {
    return trace_pixels_impl(c, u, e, pixels_dev, n_pixels, out_dev, stats, false, nullptr);
}

int mm_trace_pixels_var(mm_ctx* c, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels_dev, uint64_t n_pixels,
                        void* out_dev, float* var_dev, mm_stats* stats) {
    return trace_pixels_impl(c, u, e, pixels_dev, n_pixels, out_dev, stats, true, var_dev);
}

// The pixel lists of several frames in one launch: mm_trace_pixels' checks in its order, the plan
// (mm_plan.h plan_pixel_lists), the list table staged ahead of the launch, one kList == 2 launch and, with
// staged samples, one resolve over the concatenation as ONE list (its slots are global entry * spp + sample).
// MM_PIPE_REFERENCE: one unchanged k_trace_mega list launch per non-empty list, each into its own slice of
// the staged samples, and the same resolve.  var_dev: the variance call (mm_trace_pixels_var's conditions).
int mm_trace_pixel_lists(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const mm_ext* e,
                         const uint32_t* frame_keys, uint32_t n_lists, const uint32_t* pixels_dev,
                         const uint64_t* offsets, void* out_dev, float* var_dev, mm_stats* stats) {
    if (!c) return MM_ERR_INVALID;
    const char* fn = "mm_trace_pixel_lists";
    const bool var_call = var_dev != nullptr;
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_trace_pixel_lists: no scene uploaded");
    uint64_t n_entries = 0;
    std::string why;
    if (int rc0 = lists_total(offsets, n_lists, n_entries, why)) return fail(c, rc0, why);
    if (n_entries == 0) return MM_OK;
    if (!u || !e || !pixels_dev || !out_dev) return fail(c, MM_ERR_INVALID, "mm_trace_pixel_lists: null argument");
    if (int rc0 = check_tile(c, fn, u, e, e->mirror_limit, 0, 0, 1, 1, 1)) return rc0;
    const bool rgba8 = (e->flags & MM_EXT_RGBA8) != 0;
    if (rgba8 && (e->flags & MM_EXT_ACCUMULATE))
        return fail(c, MM_ERR_INVALID, "mm_trace_pixel_lists: MM_EXT_RGBA8 results cannot accumulate");
    const size_t out_bpp = rgba8 ? 4 : 16;
    if (reinterpret_cast<uintptr_t>(pixels_dev) % 8 || reinterpret_cast<uintptr_t>(out_dev) % out_bpp)
        return fail(c, MM_ERR_INVALID, std::string("mm_trace_pixel_lists: lists not 8-byte or output not ") +
                                           std::to_string(out_bpp) + "-byte aligned");
    if (var_call) {
        if (n_entries > 0xFFFFFFFFull)  // (the plan's own refusal, ahead of the byte counts below)
            return fail(c, MM_ERR_INVALID, "mm_trace_pixel_lists: more paths than one launch holds (2^32)");
        if (int rc0 = check_var(c, fn, e, out_dev, n_entries * out_bpp, var_dev, n_entries)) return rc0;
    }
    HIPC(c, hipSetDevice(c->device));
    const bool want_stats = (e->flags & MM_EXT_COUNT_STATS) != 0;
    const bool persist = c->pipe != MM_PIPE_REFERENCE && c->opt_persist == 2;
    const SceneFacts facts = scene_facts(c);
    PlanOptions opts = plan_options(c);
    if (var_call) opts.opt_fuse = false;  // the variance is taken of the staged samples
    const ListsPlan lp = plan_pixel_lists(opts, *e, offsets, n_lists);
    if (lp.plan.code != MM_OK) return fail(c, lp.plan.code, lp.plan.error);
    int form = 0, mode = 0;
    if (persist) {
        Choice m = choose_method(facts, opts);
        if (m.code == MM_OK) m = choose_placement(facts, opts, m.form);
        if (m.code != MM_OK) return fail(c, m.code, m.error);
        form = m.form;
        mode = m.mode;
    }
    const bool fuse = lp.plan.fuse;
    int rc = fuse ? MM_OK : ensure(c, c->d_samples, c->samples_cap, (size_t)(n_entries * e->spp));
    if (rc) return rc;
    auto key_of = [&](uint32_t f) { return frame_keys ? frame_keys[f] : e->frame + f; };
    auto cam_of = [&](uint32_t f) -> const mm_camera& { return cams ? cams[f] : u->cam; };
    const uint32_t* table_dev = nullptr;
    if (persist) {
        rc = stage_lists(c, ListTable::words(n_lists), [&](uint32_t* t) {
            const uintptr_t px = reinterpret_cast<uintptr_t>(pixels_dev);
            t[ListTable::kPixLo] = (uint32_t)px;
            t[ListTable::kPixHi] = (uint32_t)((uint64_t)px >> 32);
            t[ListTable::kLists] = n_lists;
            t[ListTable::kChunks] = lp.n_chunks;
            t[ListTable::kRecords] = ListTable::records_at(n_lists);
            for (uint32_t f = 0; f < n_lists; ++f) {
                const ListSpan& l = lp.lists[f];
                t[ListTable::kHeader + f] = l.first_chunk;
                uint32_t* r = t + ListTable::records_at(n_lists) + (size_t)f * ListTable::kRecWords;
                std::memcpy(r, &cam_of(f), sizeof(mm_camera));
                r[ListTable::kKey] = key_of(f);
                r[ListTable::kFirstChunk] = l.first_chunk;
                r[ListTable::kNumChunks] = l.n_chunks;
                r[ListTable::kFirstEntry] = l.first_entry;
                r[ListTable::kPaths] = l.n_paths;
                r[ListTable::kEntries] = l.n_entries;
            }
            t[ListTable::kHeader + n_lists] = lp.n_chunks;
        }, table_dev);
        if (rc) return rc;
    }
    if (want_stats) HIPC(c, hipMemsetAsync(c->d_aux, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = begin_timing(c))) return rc;
    uint32_t* err_dev = reinterpret_cast<uint32_t*>(c->d_aux + 4);
    const DevScene sc = dev_scene(c);
    // the concatenation as one list: the resolve's job, and the base of the launches'
    TileJob all;
    all.u = *u;
    all.e = *e;
    all.x0 = 0;
    all.y0 = 0;
    all.w = (uint32_t)n_entries;
    all.h = 1;
    all.y_stride = 1;
    all.view_w = (uint32_t)u->view_w;
    all.fuse = fuse ? 1u : 0u;
    all.wave_ts = c->d_wave_ts;
    all.wave_ts_cap = c->wave_ts_cap;
    all.out = out_dev;
    all.reserve_cus = c->opt_reserve_cus;
    all.predraw = lp.plan.predraw;
    all.predraw_pool = lp.plan.predraw_pool;
    all.fault = c->opt_fault == 1 ? 1u : 0u;
    all.ring_diag = c->d_status + kStatusSlots;
    all.list = 1;
    all.pixels = reinterpret_cast<const uint2*>(pixels_dev);
    c->calls.begin_call();
    uint32_t launches = 0;
    if (persist) {
        TileJob job = all;
        job.list = 2;
        job.lists = table_dev;
        rc = enqueue_launch(c, true, [&](uint32_t* status, uint32_t launch_id) -> int {
            job.status = status;
            job.launch_id = launch_id;
            if (c->opt_fault == 3) return fail(c, MM_ERR_HIP, "injected enqueue failure (MM_OPT_FAULT_INJECT 3)");
            c->last_form = form >= kFormGrid ? kFormGrid : form;
            c->last_mode = mode;
            c->last_kern_mode = mode;
            c->last_kern_form = form;
            c->last_kern_ring = 0;
            HIPC(c, launch_trace_wavepersist(sc, job, c->d_samples, c->d_aux, err_dev, c->d_work, want_stats, mode,
                                             form, c->stream));
            return MM_OK;
        });
        if (!rc) ++launches;
    } else {
        for (uint32_t f = 0; f < n_lists && !rc; ++f) {
            const ListSpan& l = lp.lists[f];
            if (!l.n_entries) continue;
            TileJob job = all;
            job.u.cam = cam_of(f);
            job.e.frame = key_of(f);
            job.w = l.n_entries;
            job.pixels = all.pixels + l.first_entry;
            job.out = reinterpret_cast<char*>(out_dev) + (size_t)l.first_entry * out_bpp;
            Sample* samples = c->d_samples + (size_t)l.first_entry * e->spp;
            rc = enqueue_launch(c, false, [&](uint32_t* status, uint32_t launch_id) -> int {
                job.status = status;
                job.launch_id = launch_id;
                if (c->opt_fault == 3) return fail(c, MM_ERR_HIP, "injected enqueue failure (MM_OPT_FAULT_INJECT 3)");
                MegaOpts mo;
                mo.reference = true;
                mo.block = c->opt_block ? c->opt_block : 256u;
                HIPC(c, launch_trace_mega(sc, job, samples, c->d_aux, err_dev, want_stats, mo, c->stream));
                return MM_OK;
            });
            if (!rc) ++launches;
        }
    }
    if (!rc && !fuse) {
        const hipError_t re = var_call ? launch_resolve_var(all, c->d_samples, out_dev, var_dev, c->stream)
                                       : launch_resolve(all, c->d_samples, out_dev, c->stream);
        if (re != hipSuccess) rc = fail(c, MM_ERR_HIP, std::string("launch_resolve: ") + hipGetErrorString(re));
        ++launches;
    }
    c->last_defer = false;
    char what[160] = "";
    if (c->calls.call_has_launches())
        snprintf(what, sizeof(what), "%s, %u lists, %llu pixels, %u spp", fn, n_lists, (unsigned long long)n_entries,
                 e->spp);
    c->calls.end_call(what);
    if (rc) return rc;
    if ((rc = end_timing(c, launches))) return rc;
    if (want_stats) {
        if ((rc = read_aux(c, stats))) return rc;
        return report_failure(c, "");
    }
    return MM_OK;
}

namespace {

// Query policy of mm_query_rays / mm_trace_aov (aov_kernels.hip): the method the trace calls would take for
// the scene and MM_OPT_TRAVERSAL (mm_plan.h choose_method), without their LDS placements -- those kernels
// read the scene from global memory, where every grid form and both BVH forms exist.
int aov_policy(mm_ctx* c, int& policy) {
    if (c->pipe == MM_PIPE_REFERENCE) {
        policy = kAovRef;
        return MM_OK;
    }
    const Choice m = choose_method(scene_facts(c), plan_options(c));
    if (m.code != MM_OK) return fail(c, m.code, m.error);
    if (grid_form(m.form))
        policy = kAovGrid + (grid_slow(m.form) ? kAovGridSlow : 0) + (grid_wide(m.form) ? kAovGridWide : 0) +
                 (grid_flat(m.form) ? kAovGridFlat : 0);
    else
        policy = m.form == kFormLean ? kAovBvhLean : kAovBvhLi;
    if (!aov_policy_built(policy))
        return fail(c, MM_ERR_UNSUPPORTED, "query policy " + std::to_string(policy) + " not built");
    return MM_OK;
}

// One numbered call of one kernel launch (a non-persistent kernel: its error flag is published into the
// call's status word by a launch of its own).  launch(err_dev) enqueues the kernel.
extern "C++" template <typename L>
int enqueue_query_call(mm_ctx* c, const std::string& what, const char* name, L&& launch) {
    int rc = begin_timing(c);
    if (rc) return rc;
    c->calls.begin_call();
    rc = enqueue_launch(c, false, [&](uint32_t*, uint32_t) -> int {
        const hipError_t le = launch(reinterpret_cast<uint32_t*>(c->d_aux + 4));
        return le == hipSuccess ? MM_OK : fail(c, MM_ERR_HIP, std::string(name) + ": " + hipGetErrorString(le));
    });
    c->calls.end_call(what);
    if (rc) return rc;
    return end_timing(c, 2);
}

}  // namespace

int mm_query_rays(mm_ctx* c, const float* rays_dev, uint64_t n_rays, void* hits_dev) {
    if (!c) return MM_ERR_INVALID;
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_query_rays: no scene uploaded");
    if (n_rays == 0) return MM_OK;
    if (!rays_dev || !hits_dev) return fail(c, MM_ERR_INVALID, "mm_query_rays: null argument");
    if (reinterpret_cast<uintptr_t>(rays_dev) % 16 || reinterpret_cast<uintptr_t>(hits_dev) % 8)
        return fail(c, MM_ERR_INVALID, "mm_query_rays: rays not 16-byte or hits not 8-byte aligned");
    if (n_rays > aov_max_items()) return fail(c, MM_ERR_INVALID, "mm_query_rays: more rays than one launch holds");
    HIPC(c, hipSetDevice(c->device));
    int policy = 0;
    if (int rc = aov_policy(c, policy)) return rc;
    const DevScene sc = dev_scene(c);
    char what[96];
    snprintf(what, sizeof(what), "mm_query_rays, %llu rays", (unsigned long long)n_rays);
    return enqueue_query_call(c, what, "launch_query_rays", [&](uint32_t* err_dev) {
        return launch_query_rays(sc, policy, reinterpret_cast<const float4*>(rays_dev), n_rays,
                                 reinterpret_cast<RayHit*>(hits_dev), err_dev, c->stream);
    });
}

int mm_trace_aov(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, uint32_t n_frames, uint32_t mirror_limit,
                 uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, const mm_aov* out) {
    if (!c) return MM_ERR_INVALID;
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_trace_aov: no scene uploaded");
    if (!u || !out) return fail(c, MM_ERR_INVALID, "mm_trace_aov: null argument");
    if (!out->normal_depth && !out->albedo && !out->id) return fail(c, MM_ERR_INVALID, "mm_trace_aov: no output");
    if (n_frames == 0) return fail(c, MM_ERR_INVALID, "mm_trace_aov: no frames");
    if (!cams && n_frames > 1) return fail(c, MM_ERR_INVALID, "mm_trace_aov: several frames need their cameras");
    if (int rc0 = check_tile(c, "mm_trace_aov", u, nullptr, mirror_limit, x0, y0, w, h, y_stride)) return rc0;
    if (reinterpret_cast<uintptr_t>(out->normal_depth) % 16 || reinterpret_cast<uintptr_t>(out->albedo) % 16 ||
        reinterpret_cast<uintptr_t>(out->id) % 4)
        return fail(c, MM_ERR_INVALID, "mm_trace_aov: float4 outputs not 16-byte or id not 4-byte aligned");
    const uint64_t n_pix = (uint64_t)w * h;
    if (n_pix > 0x7FFFFFFFull || (n_pix + 255) / 256 * n_frames > 0x7FFFFFFFull)
        return fail(c, MM_ERR_INVALID, "mm_trace_aov: more pixels than one launch holds");
    HIPC(c, hipSetDevice(c->device));
    int policy = 0;
    if (int rc = aov_policy(c, policy)) return rc;
    AovJob job;
    job.u = *u;
    job.cams = nullptr;
    if (cams)
        if (int rc = stage_cameras(c, cams, n_frames, job.cams)) return rc;
    job.n_frames = n_frames;
    job.mirror_limit = mirror_limit;
    job.x0 = x0; job.y0 = y0; job.w = w; job.h = h; job.y_stride = y_stride;
    job.normal_depth = reinterpret_cast<float4*>(out->normal_depth);
    job.albedo = reinterpret_cast<float4*>(out->albedo);
    job.id = out->id;
    const DevScene sc = dev_scene(c);
    char what[160];
    snprintf(what, sizeof(what), "mm_trace_aov, %u frames, tile (%u, %u) %ux%u / %u, mirror limit %u", n_frames, x0,
             y0, w, h, y_stride, mirror_limit);
    return enqueue_query_call(c, what, "launch_trace_aov", [&](uint32_t* err_dev) {
        return launch_trace_aov(sc, policy, job, err_dev, c->stream);
    });
}

int mm_sync(mm_ctx* c) {
    if (!c) return MM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (int rc = read_aux(c, nullptr)) return rc;
    return report_failure(c, "");
}

int mm_last_call(const mm_ctx* c, uint64_t* call_id) {
    if (!c || !call_id) return MM_ERR_INVALID;
    *call_id = c->calls.last_call();
    return MM_OK;
}

int mm_call_status(mm_ctx* c, uint64_t call_id) {
    if (!c) return MM_ERR_INVALID;
    return c->calls.call_status(call_id, c->err);
}

int mm_set_profiling(mm_ctx* c, int enable) {
    if (!c) return MM_ERR_INVALID;
    c->prof = enable != 0;
    return MM_OK;
}

int mm_kernel_timing(mm_ctx* c, float* total_ms, uint32_t* launches, int reset) {
    if (!c) return MM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    float sum = 0.0f;
    for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
        float ms = 0.0f;
        HIPC(c, hipEventSynchronize(c->prof_ev[i + 1]));
        HIPC(c, hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]));
        sum += ms;
    }
    if (total_ms) *total_ms = sum;
    if (launches) *launches = (uint32_t)(c->prof_used / 2);
    if (reset) c->prof_used = 0;
    return MM_OK;
}

int mm_last_timing(mm_ctx* c, float* ms, uint32_t* launches) {
    if (!c) return MM_ERR_INVALID;
    if (c->last_ms < 0.0f) {
        HIPC(c, hipEventSynchronize(c->ev1));
        HIPC(c, hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    }
    if (ms) *ms = c->last_ms;
    if (launches) *launches = c->last_launches;
    return MM_OK;
}

}  // extern "C"
