// mm_runtime.hip — the C ABI of include/mm_api.h over the HIP runtime: the context, its options, the scene,
// the parity path (mm_trace_chunks, present, read-backs), sync, status and timing.  (The trace and query calls:
// mm_trace_calls.hip; the frame filters' six calls: mm_filters.hip; the multi-GPU path: mm_comm.hip.)
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
#include "mm_api.h"
#include "mm_ctx.h"
#include "mm_launch.h"

using namespace mm;

namespace mm {
size_t build_compact_rects(const mm_rect* rects, uint32_t n_rects, const uint32_t* idx, std::vector<uint32_t>& out,
                           size_t* n_slow);
}

// The helpers the trace and query calls (mm_trace_calls.hip) share with this file: declared in mm_ctx.h.
namespace mm {

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

int order_shared(mm_ctx* c) {
    if (c->shared_done && c->shared_stream != c->stream) HIPC(c, hipStreamWaitEvent(c->stream, c->shared_done, 0));
    return MM_OK;
}
// `done` was just recorded on the context's stream, after the last work of a call that order_shared guards.
static void shared_until(mm_ctx* c, hipEvent_t done) {
    c->shared_done = done;
    c->shared_stream = c->stream;
}

int begin_timing(mm_ctx* c) {
    HIPC(c, hipEventRecord(c->ev0, c->stream));
    return MM_OK;
}
int end_timing(mm_ctx* c, uint32_t launches) {
    HIPC(c, hipEventRecord(c->ev1, c->stream));
    shared_until(c, c->ev1);
    c->last_launches = launches;
    c->last_ms = -1.0f;  // resolved lazily in mm_last_timing
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

int report_failure(mm_ctx* c, const char* suffix) { return c->calls.report_failure(suffix, c->err); }

}  // namespace mm

namespace {

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
    for (StageRing* r : {&c->cams, &c->lists}) {
        (void)hipFree(r->dev);
        if (r->host) (void)hipHostFree(r->host);
    }
    (void)hipFree(c->d_dn_img); (void)hipFree(c->d_dn_keys); (void)hipFree(c->d_dn_var);
    if (c->dn_done) (void)hipEventDestroy(c->dn_done);
    if (c->gather_done) (void)hipEventDestroy(c->gather_done);
    if (c->present_done) (void)hipEventDestroy(c->present_done);
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
        case MM_OPT_UPSAMPLE_LDS:
            if (value < 0 || value > 1) return fail(c, MM_ERR_INVALID, "upsample LDS staging must be 0 or 1");
            c->opt_upsample_lds = value != 0;
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
        case MM_INFO_LAST_KERNEL_FORM: *value = c->last_kern_form; return MM_OK;
        case MM_INFO_LAST_RING: *value = c->last_kern_ring; return MM_OK;
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
    // the old scene goes once everything the context has queued, on any stream used so far, is done with it
    if (c->has_scene) HIPC(c, hipDeviceSynchronize());
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
    if (int rc = order_shared(c)) return rc;
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
    if (int rc = order_shared(c)) return rc;
    if (!c->present_done) HIPC(c, hipEventCreateWithFlags(&c->present_done, hipEventDisableTiming));
    HIPC(c, launch_present_blur(c->d_fb8, c->d_fb8_alt, c->fb_w, c->fb_h, c->stream));
    std::swap(c->d_fb8, c->d_fb8_alt);
    HIPC(c, hipEventRecord(c->present_done, c->stream));
    shared_until(c, c->present_done);
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
    int rc = order_shared(c);
    if (!rc) rc = ensure(c, c->d_packets, c->packets_cap, 16 * (size_t)n_chunks);
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
    if (int rc = order_shared(c)) return rc;
    if (rgba) HIPC(c, hipMemcpyAsync(rgba, c->d_fb, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (rgba8) HIPC(c, hipMemcpyAsync(rgba8, c->d_fb8, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

int mm_sync(mm_ctx* c) {
    if (!c) return MM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    if (int rc = order_shared(c)) return rc;  // (the error word is read on the stream: after its last writer)
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
