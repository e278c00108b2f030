// mm_trace_calls.hip — the numbered calls of the C ABI (include/mm_api.h): the eight trace calls
// (mm_trace_tile, _frames, _cameras, _var; mm_trace_pixels, _var; mm_trace_pixel_lists; mm_trace_rays),
// mm_trace_aov and mm_query_rays.  Every call checks its arguments first (mm_trace_args.h), then plans
// (mm_plan.h), stages what the launch reads (mm_stage_ring.h) and enqueues its launches as one call of the
// context's tracker (mm_calls.h).
//
// The steps the trace calls share stand once -- kernel choice, base job, one launch, resolve, close of the call
// -- under two bodies: the tile calls' (row batches, deferral, cameras) and the list calls'.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "mm_aov.h"
#include "mm_api.h"
#include "mm_ctx.h"
#include "mm_launch.h"
#include "mm_plan.h"
#include "mm_trace_args.h"

using namespace mm;

namespace {

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

// The tail rings' records (mm_launch.h TailQueue): kTailRing per resident
// block, at most 2 blocks per CU.
int tail_queue(mm_ctx* c, TailQueue& q) {
    int cus = 0;
    HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const uint32_t cap = 2u * (uint32_t)cus * kTailRing;
    if (c->tail_cap < cap || !c->d_tail) {
        if (c->d_tail) HIPC(c, hipDeviceSynchronize());  // (a queued launch may still use the old rings: ensure_idle)
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

// `words` fresh words of a staging ring (mm_stage_ring.h: where they lie, and when the device is waited for and
// the ring grown, is ring_place's), zeroed, written by fill(host words) and mirrored to the device by a copy on
// the context's stream, ahead of the launch that reads them at `dev`.
template <typename F>
int stage(mm_ctx* c, StageRing& r, size_t words, F&& fill, const uint32_t*& dev) {
    const RingPlace p = ring_place(r.cap, r.next, words, r.min_cap, r.wrap_cap);
    if (p.wait) HIPC(c, hipDeviceSynchronize());  // staged words may still be on their way, on any stream used so far
    if (p.grow) {
        if (r.host) (void)hipHostFree(r.host);
        (void)hipFree(r.dev);
        r.host = nullptr; r.dev = nullptr; r.cap = 0;
        HIPC(c, hipHostMalloc((void**)&r.host, p.grow * sizeof(uint32_t), hipHostMallocDefault));
        HIPC(c, hipMalloc((void**)&r.dev, p.grow * sizeof(uint32_t)));
        r.cap = p.grow;
    }
    uint32_t* h = r.host + p.at;
    std::memset(h, 0, words * sizeof(uint32_t));
    fill(h);
    uint32_t* d = r.dev + p.at;
    HIPC(c, hipMemcpyAsync(d, h, words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    r.next = p.at + words;
    dev = d;
    return MM_OK;
}

// The device records of a camera-sequence launch (mm_launch.h TileJob::cams, mm_aov.h AovJob::cams): every call
// takes fresh records, so a later call's cameras never land on those of a launch still running.
int stage_cams(mm_ctx* c, const mm_camera* cams, uint32_t n, const float*& dev) {
    const uint32_t* words = nullptr;
    const int rc = stage(c, c->cams, (size_t)n * kCamStride, [&](uint32_t* h) {
        for (uint32_t f = 0; f < n; ++f) std::memcpy(h + (size_t)f * kCamStride, &cams[f], sizeof(mm_camera));
    }, words);
    dev = reinterpret_cast<const float*>(words);
    return rc;
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

// ---- per-call status (mm_calls.h) -------------------------------------------
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

// ---- the trace calls' shared steps ------------------------------------------
// The kernel a trace call launches: the wave-persistent kernel's instance (persist: mode, form and its tail-ring
// kind, 0 in a list call), else MM_PIPE_REFERENCE's one thread per path.
struct TraceKernel {
    bool persist = false;
    int form = 0, mode = 0, ring = 0;
    bool want_stats = false;
    DevScene sc;
};

// Kernel choice: the query method and its LDS placement (mm_plan.h), or the refusal.
int choose_kernel(mm_ctx* c, const SceneFacts& facts, const PlanOptions& opts, TraceKernel& k) {
    k.persist = c->pipe != MM_PIPE_REFERENCE;
    if (!k.persist) return MM_OK;
    Choice m = choose_method(facts, opts);
    if (m.code == MM_OK) m = choose_placement(facts, opts, m.form);
    if (m.code != MM_OK) return fail(c, m.code, m.error);
    k.form = m.form;
    k.mode = m.mode;
    return MM_OK;
}

// Base job: what every launch of a call takes from the context, the call's u / e, its plan and `out`.  The
// tile itself (x0, y0, w, h, y_stride) is the caller's.
TileJob base_job(const mm_ctx* c, const mm_uniform& u, const mm_ext& e, const LaunchPlan& plan, void* out) {
    TileJob job;
    job.u = u;
    job.e = e;
    job.view_w = (uint32_t)u.view_w;
    job.fuse = plan.fuse ? 1u : 0u;
    job.wave_ts = c->d_wave_ts;
    job.wave_ts_cap = c->wave_ts_cap;
    job.out = out;
    job.reserve_cus = c->opt_reserve_cus;
    job.predraw = plan.predraw;
    job.predraw_pool = plan.predraw_pool;
    job.fault = c->opt_fault == 1 ? 1u : 0u;
    job.ring_diag = c->d_status + kStatusSlots;
    return job;
}

// One launch of the open call: the job gets its status word and launch id, then the kernel is enqueued.
// aux: [0..3] stats (zeroed only when counted), [4] error flag (moved into the launch's status word by
// the launch itself).  d_work: the wave-persistent kernel's queue head(s) and waves-done word
// (self-cleaning).  No fill kernel on the default path: see k_trace_wavepersist.
int enqueue_trace(mm_ctx* c, const TraceKernel& k, TileJob& job, Sample* samples) {
    return enqueue_launch(c, k.persist, [&](uint32_t* status, uint32_t launch_id) -> int {
        uint32_t* err_dev = reinterpret_cast<uint32_t*>(c->d_aux + 4);
        job.status = status;
        job.launch_id = launch_id;
        if (c->opt_fault == 3) return fail(c, MM_ERR_HIP, "injected enqueue failure (MM_OPT_FAULT_INJECT 3)");
        if (k.persist) {
            c->last_form = k.form >= kFormGrid ? kFormGrid : k.form;
            c->last_mode = k.mode;
            c->last_kern_mode = k.mode;
            c->last_kern_form = k.form;
            c->last_kern_ring = k.ring;
            HIPC(c, launch_trace_wavepersist(k.sc, job, samples, c->d_aux, err_dev, c->d_work, k.want_stats, k.mode,
                                             k.form, c->stream));
        } else {
            MegaOpts mo;
            mo.reference = true;
            mo.block = c->opt_block ? c->opt_block : 256u;
            HIPC(c, launch_trace_mega(k.sc, job, samples, c->d_aux, err_dev, k.want_stats, mo, c->stream));
        }
        return MM_OK;
    });
}

// Resolve of the staged samples of `rj` into `out`; var: and their variance beside it (a variance call).
int enqueue_resolve(mm_ctx* c, const TileJob& rj, void* out, float* var) {
    const hipError_t re = var ? launch_resolve_var(rj, c->d_samples, out, var, c->stream)
                              : launch_resolve(rj, c->d_samples, out, c->stream);
    if (re != hipSuccess) return fail(c, MM_ERR_HIP, std::string("launch_resolve: ") + hipGetErrorString(re));
    return MM_OK;
}

// Close of the call: `what` names it to the tracker (for the launches it enqueued: all of them unless rc).
int end_trace_call(mm_ctx* c, int rc, bool defer, const char* what, uint32_t launches, bool want_stats,
                   mm_stats* stats) {
    c->last_defer = defer;
    c->calls.end_call(what);
    // (after a failure too: the launches the call did enqueue are what a call on another stream waits for)
    const int te = end_timing(c, launches);
    if (rc) return rc;
    if (te) return te;
    if (want_stats) {
        if ((rc = read_aux(c, stats))) return rc;
        return report_failure(c, "");  // (synced: this call's own error, if any)
    }
    return MM_OK;
}

// ---- the tile calls ----------------------------------------------------------
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
    const ArgCheck ck = check_trace_tile(fn, var_call, u, e, n_frames, x0, y0, w, h, y_stride, out_dev, var_dev);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    const size_t out_bpp = (e->flags & MM_EXT_RGBA8) ? 4 : 16;
    HIPC(c, hipSetDevice(c->device));
    // the plan (mm_plan.h): query method and LDS placement, then deferral / ring kind / fused resolve / rows
    // per launch, given the static LDS of the placement's deferral kernels
    const SceneFacts facts = scene_facts(c);
    PlanOptions opts = plan_options(c);
    if (var_call) opts.opt_fuse = false;  // the variance is taken of the staged samples
    TraceKernel k;
    k.want_stats = (e->flags & MM_EXT_COUNT_STATS) != 0;
    if (int rc0 = choose_kernel(c, facts, opts, k)) return rc0;
    size_t static_lds[2] = {kNotBuilt, kNotBuilt};
    if (k.persist && wavepersist_defer_built(k.mode, k.form) && (c->opt_defer != 0 || c->pipe == MM_PIPE_WAVEFRONT))
        for (int kind : {1, 2}) {
            hipFuncAttributes a{};
            // (a static-grid placement is fitted to the array's capacity: the kernel's own figure is not read)
            if (lds_static_grid(k.mode)) static_lds[kind - 1] = 0;
            else if (wavepersist_attributes(k.mode, k.form, kind, &a) == hipSuccess)
                static_lds[kind - 1] = a.sharedSizeBytes;
        }
    const LaunchPlan plan =
        plan_tile(facts, opts, k.form, k.mode, static_lds, *e, w, h, n_frames, multi ? fn : nullptr);
    if (plan.code != MM_OK) return fail(c, plan.code, plan.error);
    k.ring = plan.ring;
    const bool defer = plan.defer, fuse = plan.fuse;
    const uint32_t rows_per_batch = plan.rows_per_batch;
    const uint64_t row_paths = (uint64_t)w * e->spp;
    int rc = fuse ? MM_OK : ensure_idle(c, c->d_samples, c->samples_cap,
                                        (size_t)(row_paths * rows_per_batch) * (defer ? n_frames : 1));
    if (rc) return rc;
    TailQueue tq;
    if (defer && plan.ring == 1 && (rc = tail_queue(c, tq))) return rc;  // (records in LDS: no global ring)
    const float* cams_dev = nullptr;
    if (cams && (rc = stage_cams(c, cams, n_frames, cams_dev))) return rc;
    if ((rc = order_shared(c))) return rc;
    if (k.want_stats) HIPC(c, hipMemsetAsync(c->d_aux, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = begin_timing(c))) return rc;
    k.sc = dev_scene(c);
    c->calls.begin_call();
    uint32_t launches = 0;
    for (uint32_t j0 = 0; j0 < h; j0 += rows_per_batch) {
        TileJob job = base_job(c, *u, *e, plan, reinterpret_cast<char*>(out_dev) + (size_t)j0 * w * out_bpp);
        job.x0 = x0;
        job.y0 = y0 + j0 * y_stride;
        job.w = w;
        job.h = std::min(rows_per_batch, h - j0);
        job.y_stride = y_stride;
        job.n_frames = n_frames;
        job.cams = cams_dev;
        if (c->opt_fault == 4) job.fault = 4;
        if (c->opt_fault == 2) job.ring_spin = 0;
        if (defer) {
            job.defer_from = 1;
            job.defer_lanes = c->opt_defer > 0 ? (uint32_t)c->opt_defer : 32u;
            job.tail = tq;
            job.ring_lds = plan.ring == 2 ? 1u : 0u;
        }
        if ((rc = enqueue_trace(c, k, job, c->d_samples))) break;
        launches += fuse ? 1 : 2;
        if (fuse) continue;
        // the frames' staged samples and output slices are contiguous (a multi-frame launch is one
        // row batch), so one resolve over h x n_frames rows covers them all
        TileJob rj = job;
        if (defer) rj.h = job.h * n_frames;
        // (a later row batch's variances start at its own rows)
        if ((rc = enqueue_resolve(c, rj, job.out, var_call ? var_dev + (size_t)j0 * w : nullptr))) break;
    }
    char what[160];
    snprintf(what, sizeof(what), "%s, frames %u..%u, tile (%u, %u) %ux%u / %u, %u spp",
             var_call ? "mm_trace_tile_var" : multi ? fn : "mm_trace_tile", e->frame, e->frame + n_frames - 1, x0, y0,
             w, h, y_stride, e->spp);
    return end_trace_call(c, rc, defer, what, launches, k.want_stats, stats);
}

// ---- the list calls ----------------------------------------------------------
// The launch path the list calls share (pixel lists, ray lists), after their checks and their plan -- whose
// refusals (the queue and staging bounds) need no kernel: the kernel choice, the staged samples, prep(k) -- what
// the launch reads, staged on the stream ahead of it --, and one numbered call over the base job `all`, a
// one-row tile n_entries wide: launch(k, all, launches) names the job's source and enqueues the call's trace
// launches; with staged samples one resolve follows, over all entries (slot entry * spp + sample); var_dev: and
// their variance.
template <typename Prep, typename Launch>
int list_call(mm_ctx* c, const PlanOptions& opts, const LaunchPlan& plan, const mm_uniform& u, const mm_ext& e,
              uint64_t n_entries, void* out_dev, float* var_dev, mm_stats* stats, const char* what, Prep&& prep,
              Launch&& launch) {
    TraceKernel k;
    k.want_stats = (e.flags & MM_EXT_COUNT_STATS) != 0;
    if (int rc0 = choose_kernel(c, scene_facts(c), opts, k)) return rc0;
    const bool fuse = plan.fuse;
    int rc = fuse ? MM_OK : ensure_idle(c, c->d_samples, c->samples_cap, (size_t)(n_entries * e.spp));
    if (rc) return rc;
    if ((rc = prep(k))) return rc;
    if ((rc = order_shared(c))) return rc;
    if (k.want_stats) HIPC(c, hipMemsetAsync(c->d_aux, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = begin_timing(c))) return rc;
    k.sc = dev_scene(c);
    TileJob all = base_job(c, u, e, plan, out_dev);
    all.x0 = 0;
    all.y0 = 0;
    all.w = (uint32_t)n_entries;
    all.h = 1;
    all.y_stride = 1;
    c->calls.begin_call();
    uint32_t launches = 0;
    rc = launch(k, all, launches);
    if (!rc && !fuse) {
        TileJob rj = all;
        if (rj.list == kListRays) rj.list = 0;  // a ray list names no pixels: the tile's resolve, w = n_rays
        rc = enqueue_resolve(c, rj, out_dev, var_dev);
        ++launches;
    }
    return end_trace_call(c, rc, false, what, launches, k.want_stats, stats);
}

// The pixel lists of several frames in one launch (lists: mm_trace_pixel_lists), and one list of one frame
// (mm_trace_pixels / _var: offsets = {0, n_pixels}, no cameras, no keys): the checks, the plan (mm_plan.h
// plan_pixel_lists; the one-list calls' is plan_pixels, whose texts are theirs) and list_call over the
// concatenation of the lists: kList == 2 with the list table staged ahead of it, kList == 1 for the one list,
// which needs no table.  With staged samples, one resolve over the concatenation as ONE list.
// MM_PIPE_REFERENCE: one unchanged k_trace_mega list launch per non-empty list, each into its own slice of the
// staged samples, and the same resolve.  var_call: the variance call (mm_trace_pixels_var's conditions; as in
// trace_tile_impl).
int trace_lists_impl(mm_ctx* c, bool lists, bool var_call, const mm_uniform* u, const mm_camera* cams,
                     const mm_ext* e, const uint32_t* frame_keys, uint32_t n_lists, const uint32_t* pixels_dev,
                     const uint64_t* offsets, void* out_dev, float* var_dev, mm_stats* stats) {
    if (!c) return MM_ERR_INVALID;
    const char* fn = lists ? "mm_trace_pixel_lists" : "mm_trace_pixels";
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, std::string(fn) + ": no scene uploaded");
    uint64_t n_entries = 0;
    const ArgCheck ck =
        check_trace_lists(lists, var_call, u, e, offsets, n_lists, pixels_dev, out_dev, var_dev, n_entries);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (n_entries == 0) return MM_OK;
    const size_t out_bpp = (e->flags & MM_EXT_RGBA8) ? 4 : 16;
    HIPC(c, hipSetDevice(c->device));
    PlanOptions opts = plan_options(c);
    if (var_call) opts.opt_fuse = false;  // the variance is taken of the staged samples
    ListsPlan lp;
    if (lists) lp = plan_pixel_lists(opts, *e, offsets, n_lists);
    else lp.plan = plan_pixels(opts, *e, n_entries);
    if (lp.plan.code != MM_OK) return fail(c, lp.plan.code, lp.plan.error);
    if (!lists) {  // the accepted plan, as one span
        ListSpan one;
        one.n_entries = (uint32_t)n_entries;
        one.n_paths = one.n_entries * e->spp;
        one.n_chunks = (one.n_paths + 63u) / 64u;
        lp.lists.assign(1, one);
    }
    auto key_of = [&](uint32_t f) { return frame_keys ? frame_keys[f] : e->frame + f; };
    auto cam_of = [&](uint32_t f) -> const mm_camera& { return cams ? cams[f] : u->cam; };
    const uint32_t* table_dev = nullptr;
    char what[160];
    if (lists)
        snprintf(what, sizeof(what), "%s, %u lists, %llu pixels, %u spp", fn, n_lists, (unsigned long long)n_entries,
                 e->spp);
    else
        snprintf(what, sizeof(what), "%s, frame %u, %llu pixels, %u spp", var_call ? "mm_trace_pixels_var" : fn,
                 e->frame, (unsigned long long)n_entries, e->spp);
    return list_call(
        c, opts, lp.plan, *u, *e, n_entries, out_dev, var_call ? var_dev : nullptr, stats, what,
        [&](const TraceKernel& k) -> int {
            if (!k.persist || !lists) return MM_OK;
            // (a multiple of 16 words, so every table starts on a 64-byte line)
            return stage(c, c->lists, ListTable::words(n_lists), [&](uint32_t* t) {
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
        },
        [&](const TraceKernel& k, TileJob& all, uint32_t& launches) -> int {
            // the concatenation as one list whose pixels the list names: the resolve's job, and the base of the
            // launches'
            all.list = 1;
            all.pixels = reinterpret_cast<const uint2*>(pixels_dev);
            int rc = MM_OK;
            if (k.persist) {
                TileJob job = all;
                if (lists) {
                    job.list = 2;
                    job.lists = table_dev;
                }
                rc = enqueue_trace(c, k, job, c->d_samples);
                if (!rc) ++launches;
                return rc;
            }
            for (uint32_t f = 0; f < n_lists && !rc; ++f) {
                const ListSpan& l = lp.lists[f];
                if (!l.n_entries) continue;
                TileJob job = all;
                job.u.cam = cam_of(f);
                job.e.frame = key_of(f);
                job.w = l.n_entries;
                job.pixels = all.pixels + l.first_entry;
                job.out = reinterpret_cast<char*>(out_dev) + (size_t)l.first_entry * out_bpp;
                rc = enqueue_trace(c, k, job, c->d_samples + (size_t)l.first_entry * e->spp);
                if (!rc) ++launches;
            }
            return rc;
        });
}

// mm_trace_rays: the ray list (kList == 3), one launch in either pipe.  No uni: the job's is zero and unread.
int trace_rays_impl(mm_ctx* c, const mm_ext* e, uint32_t ray_flags, const float* rays_dev, uint64_t n_rays,
                    void* out_dev, float* var_dev, mm_stats* stats) {
    if (!c) return MM_ERR_INVALID;
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_trace_rays: no scene uploaded");
    const ArgCheck ck = check_trace_rays(e, ray_flags, rays_dev, n_rays, out_dev, var_dev);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (n_rays == 0) return MM_OK;
    HIPC(c, hipSetDevice(c->device));
    PlanOptions opts = plan_options(c);
    if (var_dev) opts.opt_fuse = false;  // the variance is taken of the staged samples
    const LaunchPlan plan = plan_rays(opts, *e, n_rays);
    if (plan.code != MM_OK) return fail(c, plan.code, plan.error);
    char what[160];
    snprintf(what, sizeof(what), "mm_trace_rays, frame %u, %llu rays, %u spp", e->frame, (unsigned long long)n_rays,
             e->spp);
    return list_call(
        c, opts, plan, mm_uniform{}, *e, n_rays, out_dev, var_dev, stats, what,
        [](const TraceKernel&) -> int { return MM_OK; },
        [&](const TraceKernel& k, TileJob& all, uint32_t& launches) -> int {
            all.list = kListRays;
            all.rays = reinterpret_cast<const float4*>(rays_dev);
            all.ray_jitter = (ray_flags & MM_RAYS_JITTER) ? 1u : 0u;
            const int rc = enqueue_trace(c, k, all, c->d_samples);
            if (!rc) ++launches;
            return rc;
        });
}

// ---- the query calls ---------------------------------------------------------
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
template <typename L>
int enqueue_query_call(mm_ctx* c, const std::string& what, const char* name, L&& launch) {
    int rc = order_shared(c);
    if (!rc) rc = begin_timing(c);
    if (rc) return rc;
    c->calls.begin_call();
    rc = enqueue_launch(c, false, [&](uint32_t*, uint32_t) -> int {
        const hipError_t le = launch(reinterpret_cast<uint32_t*>(c->d_aux + 4));
        return le == hipSuccess ? MM_OK : fail(c, MM_ERR_HIP, std::string(name) + ": " + hipGetErrorString(le));
    });
    c->calls.end_call(what);
    const int te = end_timing(c, 2);  // (after a failure too, as in end_trace_call)
    return rc ? rc : te;
}

}  // namespace

extern "C" {

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

int mm_trace_pixels(mm_ctx* c, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels_dev, uint64_t n_pixels,
                    void* out_dev, mm_stats* stats) {
    const uint64_t offsets[2] = {0, n_pixels};
    return trace_lists_impl(c, false, false, u, nullptr, e, nullptr, 1, pixels_dev, offsets, out_dev, nullptr, stats);
}

int mm_trace_pixels_var(mm_ctx* c, const mm_uniform* u, const mm_ext* e, const uint32_t* pixels_dev, uint64_t n_pixels,
                        void* out_dev, float* var_dev, mm_stats* stats) {
    const uint64_t offsets[2] = {0, n_pixels};
    return trace_lists_impl(c, false, true, u, nullptr, e, nullptr, 1, pixels_dev, offsets, out_dev, var_dev, stats);
}

int mm_trace_pixel_lists(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const mm_ext* e,
                         const uint32_t* frame_keys, uint32_t n_lists, const uint32_t* pixels_dev,
                         const uint64_t* offsets, void* out_dev, float* var_dev, mm_stats* stats) {
    return trace_lists_impl(c, true, var_dev != nullptr, u, cams, e, frame_keys, n_lists, pixels_dev, offsets, out_dev,
                            var_dev, stats);
}

int mm_trace_rays(mm_ctx* c, const mm_ext* e, uint32_t ray_flags, const float* rays_dev, uint64_t n_rays,
                  void* out_dev, float* var_dev, mm_stats* stats) {
    return trace_rays_impl(c, e, ray_flags, rays_dev, n_rays, out_dev, var_dev, stats);
}

int mm_query_rays(mm_ctx* c, const float* rays_dev, uint64_t n_rays, void* hits_dev) {
    if (!c) return MM_ERR_INVALID;
    if (int rc0 = report_failure(c, "; this call was not enqueued")) return rc0;
    if (!c->has_scene) return fail(c, MM_ERR_NO_SCENE, "mm_query_rays: no scene uploaded");
    const ArgCheck ck = check_query_rays(rays_dev, n_rays, hits_dev, aov_max_items());
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (n_rays == 0) return MM_OK;
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
    const ArgCheck ck = check_trace_aov(u, cams != nullptr, n_frames, mirror_limit, x0, y0, w, h, y_stride, out);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    HIPC(c, hipSetDevice(c->device));
    int policy = 0;
    if (int rc = aov_policy(c, policy)) return rc;
    AovJob job;
    job.u = *u;
    job.cams = nullptr;
    if (cams)
        if (int rc = stage_cams(c, cams, n_frames, job.cams)) return rc;
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

}  // extern "C"
