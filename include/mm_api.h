/*
 * mm_api.h — the drop-in boundary: a C ABI over the MI355X (gfx950) HIP
 * implementation of mirror-maze's per-pixel ray-trace loop.
 *
 * Reference interface replaced (all paths relative to the reference repo):
 *   - the Metal compute dispatch of `compute_shader`
 *       kernel signature        src/shaders.metal:245-259
 *       argument table binding  src/main.rs:870-883  (set_buffer 0..6,
 *                               set_bytes(4, Uniform), set_texture 0/1)
 *       dispatch                src/main.rs:884-885  (32x24 groups of 32x32)
 *   - the Metal buffer plumbing  src/utils.rs:86-102 (make_buf/copy_to_buf)
 *   - device/queue creation      src/main.rs:616-626, 638-640
 *   - the render pass's blur     src/main.rs:888-891, src/shaders.metal:214-225
 *                                (mm_present)
 *
 * Conventions: 0 on success, a negative MM_ERR_* code otherwise (message via
 * mm_last_error); no exceptions or aborts cross the ABI; host memory is owned
 * by the caller and copied; device memory is owned by the context unless a
 * function says it writes into a caller-provided device pointer.  A context is
 * bound to one GPU and is not thread-safe (the reference drives Metal from one
 * main thread too, src/main.rs:591).  All work is enqueued on the context's
 * stream; mm_sync waits for it (the reference never waits, src/main.rs:894).
 *
 * One context, several streams: the trace, query and parity-mode calls of a
 * context share device state -- one work counter, the staged samples, the tail
 * rings, the statistics and error words, the framebuffer -- so they run one
 * after the other, in the order they were made.  On one stream that is stream
 * order.  When the stream was changed in between (mm_set_stream), the new
 * stream first waits, on the device, for the end of the last such call made
 * on the other stream; the host never waits for this, and nothing is added
 * while the stream stays the same.  The caller's buffers are the caller's: a
 * call that reads what a call on another stream wrote is ordered by the
 * caller, as between any two streams.
 */
#ifndef MM_API_H
#define MM_API_H

#include "mm_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mm_ctx mm_ctx;

/* Library version, e.g. "mirror-maze-amd 0.1 gfx950". */
const char* mm_version(void);

/* Replaces Device::system_default() + new_command_queue (main.rs:616-623).
 * device: HIP ordinal.  The context owns a non-blocking stream. */
int  mm_create(int device, mm_ctx** out);
void mm_destroy(mm_ctx* ctx);
const char* mm_last_error(const mm_ctx* ctx);

/* Enqueue on a caller stream (hipStream_t passed as void*), e.g. torch's
 * current stream.  NULL is HIP's default (null) stream, as in HIP itself;
 * MM_OWN_STREAM restores the context's own non-blocking stream.  Only stores
 * the handle: the next trace, query or parity-mode call on the new stream
 * waits there for the context's last such call on the old one (see the head
 * of this file), so the context may be moved between streams without a sync
 * in between.  The streams must outlive the work enqueued on them. */
#define MM_OWN_STREAM ((void*)(intptr_t)-1)
int  mm_set_stream(mm_ctx* ctx, void* hip_stream);
/* The stream work is enqueued on (after mm_set_stream; initially the
 * context's own stream), e.g. to wrap it for torch.cuda.ExternalStream. */
int  mm_get_stream(const mm_ctx* ctx, void** hip_stream);

/* Replaces make_buf for buffers 1,2,3,5,6 (main.rs:725-730):
 *   rects      buffer 1  mirrors      n_rects x 48 B
 *   nodes      buffer 2  nodes        n_nodes x 32 B
 *   idx        buffer 3  indices      n_rects x u32
 *   is_mirror  buffer 5  materials    n_rects x 1 B (bool)
 *   emission   buffer 6  emissions    n_rects x float4
 * Copies the data; validates the tree (indices in range, stack depth <= 50).
 * On a context that already holds a scene:
 *   - a successful upload replaces it after all work the context has queued,
 *     on any stream, has finished (the call waits for the device), so calls
 *     made before the upload see the old scene and calls after it the new;
 *   - a refusal of the arguments -- MM_ERR_INVALID, MM_ERR_UNSUPPORTED, and
 *     MM_ERR_STACK for a tree too deep -- leaves the previous scene in place
 *     and usable;
 *   - a failure after that point (MM_ERR_HIP: an allocation or a copy) leaves
 *     the context without a scene (MM_ERR_NO_SCENE until the next upload).
 * The MM_OPT_GRID_* options are read here: changing one acts at the next
 * upload. */
int  mm_upload_scene(mm_ctx* ctx,
                     const mm_rect* rects, uint32_t n_rects,
                     const mm_node* nodes, uint32_t n_nodes,
                     const uint32_t* idx,
                     const uint8_t* is_mirror,
                     const float* emission);

/* ---- parity mode: the reference dispatch, bit for bit --------------------
 * Replaces copy_to_buf(chunks) + dispatch_thread_groups (main.rs:778-885).
 * Launches (view_w/2/ppc) x (view_h/2/ppc) reference threadgroups of 32x32
 * threads (ppc = chunk_w^2 = 16, 64 samples per pixel); threadgroup g reads
 * chunk origin chunks[g] (uint2, buffer 0) and writes 16 texels of the
 * context's framebuffer (the `texout` texture, RGBA; never cleared, like the
 * reference's Private screen texture).  n_chunks must cover the grid. */
int  mm_trace_chunks(mm_ctx* ctx, const mm_uniform* uni,
                     const uint32_t* chunks, uint32_t n_chunks);

/* Download the framebuffer (view_w x view_h, row-major, y down).
 * rgba_f32: 4 floats/texel before unorm quantisation (alpha = 1), or NULL;
 * rgba8:    RGBA8Unorm as the texture stores it (round-to-nearest-even of
 *           clamp(x,0,1)*255), or NULL. */
int  mm_read_framebuffer(mm_ctx* ctx, float* rgba_f32, uint8_t* rgba8);

/* One presentation step: the render pass's fragment_shader 5-tap blur of the
 * RGBA8 texture (src/main.rs:888-891, src/shaders.metal:214-225), as a Jacobi
 * step — every texel reads the previous texture, neighbours outside it read 0,
 * alpha is written as 1 — so the frame sequence is deterministic (the
 * reference blurs in place from concurrent fragments).  Operation order of
 * the compiled IR: c = (((L+R)+D)+U)*0.5 + C, then c * RN(1/3).  Acts on the
 * RGBA8 texture only (the float framebuffer keeps the traced values). */
int  mm_present(mm_ctx* ctx);

/* The per-pixel packets of the last mm_trace_chunks, in the layout of the
 * shaders.air revision's extra `device float4* pixel_data` output (the
 * streaming-tile format): packets[(c*16 + pn)*4 ..] = (r, g, b,
 * bitcast<float>(x << 16 | y)) for pixel pn = 0..15 of chunk c, x = chunk.x +
 * pn/4, y = chunk.y + pn%4; rgb is the 64-sample mean before quantisation.
 * packets: host buffer of n_chunks*16*4 floats; n_chunks <= the last dispatch's. */
int  mm_read_packets(mm_ctx* ctx, float* packets, uint32_t n_chunks);

/* Device-side RGBA8 quantisation of a float RGBA image (e.g. an mm_trace_tile
 * output) with the texture-write conversion (round-to-nearest-even of
 * clamp(x,0,1)*255, all four channels).  Queued on the context's stream. */
int  mm_quantize_rgba8(mm_ctx* ctx, const float* rgba_dev, uint8_t* rgba8_dev, uint64_t n_pixels);

/* ---- throughput mode: offline renderer ------------------------------------
 * Renders pixels (x0 + i, y0 + j*y_stride), 0<=i<w, 0<=j<h, of the frame
 * uni->view_w x uni->view_h with ext->spp samples each (1..4096),
 * ext->bounce_limit / ext->mirror_limit (0..32767; MM_ERR_INVALID otherwise),
 * RNG keyed on (pixel, sample, ext->frame) so any tiling
 * over any number of GPUs reproduces the 1-GPU image bit for bit.
 * out_dev: caller DEVICE pointer to w*h float4 (row-major over (j,i));
 * alpha = 1 (or, with MM_EXT_ACCUMULATE, += the frame value, alpha += 1).
 * With MM_EXT_RGBA8 out_dev holds w*h 4-byte RGBA8 pixels instead: the
 * texture-write conversion of that float4 (mm_quantize_rgba8's, alpha 255),
 * written by the trace's own resolve (the reference's output texture format,
 * src/main.rs:702-709, without a float frame in between); not with
 * MM_EXT_ACCUMULATE.
 * stats: optional host pointer; filled after an implicit sync when
 * MM_EXT_COUNT_STATS is set.  rays and paths are exact; node_visits and
 * rect_tests count the work of the query method that ran (BVH: interior
 * nodes expanded and rect tests; grid search: cells visited and rect tests,
 * plus the BVH walk's counts for the queries that fell back to it). */
int  mm_trace_tile(mm_ctx* ctx, const mm_uniform* uni, const mm_ext* ext,
                   uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                   uint32_t y_stride, float* out_dev, mm_stats* stats);

/* Several consecutive frames of the same tile in ONE launch: frame f (0 <=
 * f < n_frames) is traced with RNG frame ext->frame + f into out_dev + f*w*h*4
 * (out_dev: n_frames*w*h float4, frame-major; 4-byte pixels with
 * MM_EXT_RGBA8); each frame is bit-identical to
 * mm_trace_tile(..., frame = ext->frame + f).  The frames share the launch's
 * work queue, so the ~0.4 ms tail in which the last waves finish their last
 * chunks is paid once per launch instead of once per frame (throughput mode
 * for frame sequences; a frame's result is only complete when the launch is).
 * Needs the wave-persistent kernel with the fused resolve (64 % spp == 0) or
 * with the mirror-tail deferral (any spp: samples staged per frame and
 * resolved in one pass, at most 2^29 staged paths = 6 GiB per launch; over
 * that a fusable launch runs without deferral, others get MM_ERR_INVALID);
 * MM_EXT_ACCUMULATE is rejected (frames of one launch run concurrently). */
int  mm_trace_tile_frames(mm_ctx* ctx, const mm_uniform* uni, const mm_ext* ext, uint32_t n_frames,
                          uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                          uint32_t y_stride, float* out_dev, mm_stats* stats);

/* A moving-camera frame sequence in ONE launch: mm_trace_tile_frames with a
 * camera per frame.  Frame f (0 <= f < n_frames) is traced with camera cams[f]
 * and RNG frame ext->frame + f into out_dev + f*w*h*4 (4-byte pixels with
 * MM_EXT_RGBA8), and is bit-identical to mm_trace_tile called with uni->cam =
 * cams[f] and frame = ext->frame + f; stats are summed over the frames.  The
 * view size and chunk_w come from uni; uni->cam is ignored.  cams: HOST array
 * of n_frames cameras (e.g. mm_player_uniform's .cam after each
 * mm_player_step), consumed when the call returns; the context owns the device
 * copy, which is ordered on the context's stream ahead of the launch and never
 * shares records with an earlier call's launch that may still run.  Every
 * condition of mm_trace_tile_frames applies (also for n_frames = 1): the
 * wave-persistent kernel with fused resolve or tail deferral, no
 * MM_EXT_ACCUMULATE, the 2^32 queue and 2^29 staging bounds, one row batch;
 * MM_PIPE_REFERENCE returns MM_ERR_UNSUPPORTED, n_frames = 0 or cams = NULL
 * MM_ERR_INVALID.  (The reference moves its camera every frame,
 * src/main.rs:738-842, and pays one dispatch per frame.) */
int  mm_trace_tile_cameras(mm_ctx* ctx, const mm_uniform* uni, const mm_camera* cams,
                           const mm_ext* ext, uint32_t n_frames,
                           uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                           uint32_t y_stride, float* out_dev, mm_stats* stats);

/* ---- closest-hit answers for the caller ------------------------------------
 * The trace calls above return shaded, averaged colour only.  These two
 * return what the rays hit.  Both are enqueued on the context's stream like
 * the trace calls, take a call number (mm_last_call / mm_call_status / mm_sync
 * report their GPU-side errors), and run the query method MM_PIPE_AUTO and
 * MM_OPT_TRAVERSAL select for the scene -- the certified grid search with the
 * BVH walk as its fallback, or BVH loop form 7 / 5; MM_PIPE_REFERENCE: the
 * straight reference walk -- over the scene in global memory (MM_OPT_LDS_*
 * select nothing here).  Every method returns the reference walk's answer,
 * bit for bit.
 *
 * mm_query_rays: a batch of caller-supplied rays (line of sight, picking,
 * collision).  rays_dev: DEVICE pointer, 16-byte aligned, 8 floats per ray:
 * (ox, oy, oz, -, dx, dy, dz, -), the two w components ignored.  hits_dev:
 * DEVICE pointer, 8-byte aligned, per ray (float t, uint32_t k): the pair
 * intersect_bvh_iterative (src/shaders.metal:115-156) ends with when started
 * at t = 1e30 -- the closest rect k with t > 0.1 --, or (1e30f, MM_AOV_ID_MISS).
 * Any ray is allowed (origins outside the scene or on a wall, zero direction
 * components, unnormalised directions).  A ray whose traversal stack overflows
 * gets (1e30f, MM_AOV_ID_FAILED), never a wrong hit, and the call reports
 * MM_ERR_STACK.  n_rays = 0: MM_OK, nothing enqueued. */
int  mm_query_rays(mm_ctx* ctx, const float* rays_dev, uint64_t n_rays, void* hits_dev);

/* Per-pixel feature buffers (AOVs) of the tile (x0 + i, y0 + j*y_stride) of
 * mm_trace_tile, for n_frames cameras in one launch: what each pixel sees.
 * The path of the pixel-CENTRE ray (no jitter) is followed through the mirror
 * chain -- a mirror bounce is deterministic, src/shaders.metal:326-330 -- to
 * the first surface that shades diffusely, with the bounce loop's operations:
 *   ori = cam.center, dir = the primary direction, mh = 0, dist = 0; loop:
 *   query; nothing hit -> MISS.  Hit rect k at t: n = normalize(cross(v, u)),
 *   sg = sign(dot(dir, n)), dist += t; matte, or a mirror seen from behind
 *   (sg == 1) -> SURFACE; else if mh + 1 < mirror_limit: ori += t dir, dir =
 *   normalize(reflect(dir, n)), ++mh, again; else -> MIRROR_END.
 * mirror_limit: 0..32767 as mm_ext.mirror_limit; <= 1 gives plain first-hit
 * buffers.  Outputs (mm_aov: any may be NULL, not all), element f*w*h + j*w + i:
 *   normal_depth  (-sg * n, dist)            MISS: (0, 0, 0, 1e30f)
 *   albedo        (rect colour, (float)mh)   MISS: (0, 0, 0, (float)mh)
 *   id            k | MM_AOV_ID_SURFACE or k | MM_AOV_ID_MIRROR_END; MM_AOV_ID_MISS
 * bit-identical to the same loop over the reference walk.  cams: NULL (the one
 * camera uni->cam; n_frames must be 1) or a HOST array of n_frames cameras,
 * consumed on return (the staging of mm_trace_tile_cameras: back-to-back calls
 * neither wait nor share records); view size from uni.  A failed query gives
 * id MM_AOV_ID_FAILED and MM_ERR_STACK, as in mm_query_rays. */
int  mm_trace_aov(mm_ctx* ctx, const mm_uniform* uni, const mm_camera* cams, uint32_t n_frames,
                  uint32_t mirror_limit, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                  uint32_t y_stride, const mm_aov* out);

/* ---- denoising a traced frame ------------------------------------------------
 * An edge-aware a-trous filter over throughput-mode frames, guided by the
 * buffers of mm_trace_aov over the same tile and cameras: (id, mirror hits,
 * side) names the surface a pixel shows, also when it is seen in a mirror, so
 * a tap is taken only from the same surface; a depth term and a luminance term
 * weigh the taps that are.  (The reference hides its noise with the display
 * blur, mm_present, which smears across every edge.)
 *
 * color_dev: n_frames*w*h float4 (16-byte aligned), what mm_trace_tile /
 * _frames / _cameras write: element f*w*h + j*w + i.  guides: the three
 * buffers of one mm_trace_aov call, all required.  out_dev: n_frames*w*h
 * float4 (16-byte aligned); with MM_DN_RGBA8 4-byte pixels (4-byte aligned):
 * the texture-write conversion (mm_quantize_rgba8's) of the last pass's float
 * result.  The filter works in tile index space: neighbours are tile
 * neighbours, whatever y_stride the tile was traced with, and never another
 * frame's pixels.
 *
 * All arithmetic is IEEE binary32, no contraction, in the order written.
 * hk[5] = {1/16, 1/4, 3/8, 1/4, 1/16}; C is the pass's input (color_dev for
 * pass 0, else the previous pass's output); nd, al, id the guides (the same
 * for every pass); for pass i: s = 1 << i, sl = sigma_l * (1.0f / (float)s);
 * lum(q) = (0.25f*C_q.r + 0.5f*C_q.g) + 0.25f*C_q.b.  For pixel p = (x, y):
 *   S = (0,0,0); W = 0
 *   for dy = -2..2 (outer), dx = -2..2 (inner):
 *     q = (x + s*dx, y + s*dy); skip q outside [0,w) x [0,h)
 *     unless dx == 0 && dy == 0, skip q unless
 *       id_q == id_p (all 32 bits)  and  al_q.w == al_p.w  and
 *       (nd_p.x*nd_q.x + nd_p.y*nd_q.y) + nd_p.z*nd_q.z >= 0
 *     g = hk[dy+2] * hk[dx+2]
 *     if sigma_z > 0: t = (nd_p.w - nd_q.w) / (sigma_z * (nd_p.w + nd_q.w)); g = g / (1.0f + t*t)
 *     if sigma_l > 0: t = (lum(p) - lum(q)) / sl;                            g = g / (1.0f + t*t)
 *     S.c = S.c + g * C_q.c  (c = r, g, b);  W = W + g
 *   out.rgb = S / W;  out.a = C_p.a
 * (the centre tap always counts, so W > 0; defined for finite colours and
 * nd.w > 0, which the trace and AOV calls produce).
 *
 * MM_ERR_INVALID: a null context, p, input, guide or output; n_passes outside
 * 1..MM_DENOISE_MAX_PASSES; unknown flags; w, h or n_frames 0; a misaligned
 * pointer; out_dev overlapping color_dev or a guide; w*h over 2^31 - 1 or more
 * than 2^40 pixels in all.  Enqueued on the context's stream like
 * mm_quantize_rgba8; the inputs are never written.  The intermediate images
 * are context-owned scratch that grows on demand (growing waits for the
 * device once, as the camera staging does); its reuse is ordered on the
 * stream -- and by an event when the stream was changed in between -- so
 * back-to-back calls never wait on the host. */
int  mm_denoise_frames(mm_ctx* ctx, const float* color_dev, const mm_aov* guides,
                       const mm_denoise_params* p, uint32_t n_frames,
                       uint32_t w, uint32_t h, void* out_dev);

/* ---- variance-guided denoising -------------------------------------------------
 * The same a-trous filter with the luminance stop of every pixel scaled by the
 * local standard deviation of the pixel MEAN (the SVGF form), for frames whose
 * noise is uneven: mirror chains, or pixels that mm_trace_pixels_var topped up
 * to different sample counts.  The variance is carried through the passes with
 * squared weights and the last pass's is returned, so a caller can stop, refine
 * again or composite with it.
 *
 * color_dev, guides, out_dev: exactly as in mm_denoise_frames (frame-major, tile
 * index space; a tap never reads another frame; MM_DNV_RGBA8 for an RGBA8
 * out_dev).  vmean_dev: n_frames*w*h floats (4-byte aligned), the variance of
 * the pixel mean's luminance: var / count of mm_trace_tile_var, or of the merged
 * (var, count) after extra samples.  var_out_dev: n_frames*w*h floats (4-byte
 * aligned) or NULL: the variance image of the last pass.
 *
 * All arithmetic is IEEE binary32 (subnormals kept), no contraction, in the
 * order written; / and sqrtf are correctly rounded.  hk[5] and lum as in
 * mm_denoise_frames; k3[3] = {1/4, 1/2, 1/4}; C, V are the pass's input colour
 * and variance (color_dev and vmean_dev for pass 0, else the previous pass's
 * outputs); for pass i: s = 1 << i.  same(p,q):
 *   id_q == id_p (all 32 bits)  and  al_q.w == al_p.w  and
 *   (nd_p.x*nd_q.x + nd_p.y*nd_q.y) + nd_p.z*nd_q.z >= 0.
 * For pixel p = (x, y):
 *   if sigma_l > 0:      (this pixel's stop: a 3x3 of V at unit spacing in every pass)
 *     GV = 0; GW = 0
 *     for dy = -1..1 (outer), dx = -1..1 (inner):
 *       q = (x+dx, y+dy); skip q outside [0,w) x [0,h)
 *       unless dx == 0 && dy == 0, skip q unless same(p,q)
 *       g = k3[dy+1] * k3[dx+1];  GV = GV + g * V_q;  GW = GW + g
 *     slp = sigma_l * sqrtf(GV / GW) + eps_l
 *   S = (0,0,0); W = 0; SV = 0
 *   for dy = -2..2 (outer), dx = -2..2 (inner):
 *     q = (x + s*dx, y + s*dy); skip q outside [0,w) x [0,h)
 *     unless dx == 0 && dy == 0, skip q unless same(p,q)
 *     g = hk[dy+2] * hk[dx+2]
 *     if sigma_z > 0: t = (nd_p.w - nd_q.w) / (sigma_z * (nd_p.w + nd_q.w)); g = g / (1.0f + t*t)
 *     if sigma_l > 0: t = (lum(p) - lum(q)) / slp;                           g = g / (1.0f + t*t)
 *     S.c = S.c + g * C_q.c  (c = r, g, b);  W = W + g;  SV = SV + (g * g) * V_q
 *   out.rgb = S / W;  out.a = C_p.a;  Vout = SV / (W * W)
 * (defined for what mm_denoise_frames is, and finite V >= 0).  With sigma_l <= 0
 * the colour is, on all bits, mm_denoise_frames' with the same n_passes and
 * sigma_z and sigma_l = 0; with both terms off Vout is a fixed linear filter of V.
 * Vout treats the taps as independent: later passes' taps share inputs, so it
 * understates the variance of a several-pass result.
 *
 * MM_ERR_INVALID: everything mm_denoise_frames rejects; a null or misaligned
 * vmean_dev; a misaligned var_out_dev; sigma_l > 0 with eps_l not finite or not
 * > 0; unknown flags; reserved != 0; out_dev or var_out_dev overlapping an
 * input or each other.  Enqueued like mm_denoise_frames, whose scratch (and a
 * variance image per intermediate) it shares: calls of the two, on one stream
 * or several, take turns in the order they were made, without a host wait. */
int  mm_denoise_frames_var(mm_ctx* ctx, const float* color_dev, const mm_aov* guides,
                           const float* vmean_dev, const mm_denoise_var_params* p,
                           uint32_t n_frames, uint32_t w, uint32_t h,
                           void* out_dev, float* var_out_dev);

/* ---- temporal accumulation through mirror chains -----------------------------
 * Carries a history through the frames of a camera sequence: every surface of
 * the scene is matte or a perfect planar mirror, so the radiance a pixel shows
 * does not depend on the camera as long as it shows the same surface point
 * through the same mirrors.  normal_depth.w is the distance along the mirror
 * chain, so cam.center + dist * primary_dir(p) is the virtual image of pixel
 * p's surface point, the same world point for the camera of the frame before;
 * projecting it there names the pixels that showed the point, with no motion
 * vectors, and (id, mirror hits, normal, distance) confirm or refute each.
 * Where the history holds, the output is the running mean of up to n_max
 * frames; elsewhere it is the frame itself.  The output feeds
 * mm_denoise_frames unchanged (which passes alpha through).
 *
 * uni: view_w and view_h (uni->cam is ignored).  cams: a HOST array of the
 * n_frames cameras the frames and guides were traced with, copied into the
 * launches' arguments: consumed on return.  color_dev, guides: n_frames*w*h
 * elements, frame-major, what mm_trace_tile_cameras and mm_trace_aov write for
 * the window (x0, y0, w, h) with y_stride 1 (neighbours must be frame
 * neighbours; a multi-GPU caller accumulates the gathered frame).  out_dev:
 * n_frames*w*h float4; out.a is the history length N, a float >= 1.  The last
 * frame's output, guides and camera are what a later call takes as prev.
 *
 * All arithmetic is IEEE binary32, no contraction, in the order written; sqrtf
 * and / are correctly rounded.  Frame f's history frame is frame f-1's OUTPUT
 * of this call; for f = 0 it is prev, or none if prev is NULL.  Primed names
 * are the history frame's (H' its colour).  rot(q, qw, v), the rotation
 * primary_dir (shaders.metal:283) applies to its normalised direction:
 *   nq = -q;  s1 = -((nq.x*v.x + nq.y*v.y) + nq.z*v.z)
 *   c1 = (nq.y*v.z - nq.z*v.y, nq.z*v.x - nq.x*v.z, nq.x*v.y - nq.y*v.x)
 *   v1 = c1 + qw*v
 *   c2 = (v1.y*q.z - v1.z*q.y, v1.z*q.x - v1.x*q.z, v1.x*q.y - v1.y*q.x)
 *   rot = (qw*v1 + s1*q) + c2                       (per component)
 * For pixel p = (i, j) of frame f, px = x0 + i, py = y0 + j:
 *   C = color[f][p]
 *   NOHIST: out = (C.r, C.g, C.b, 1.0f)
 *   if there is no history frame, or id_p is MM_AOV_ID_MISS or MM_AOV_ID_FAILED: NOHIST
 *   d  = primary_dir(view, cams[f], px, py)       (the direction mm_trace_aov starts pixel p with)
 *   X  = cam.center + nd_p.w * d                  (per component: one multiply, one add)
 *   r  = X - cam'.center
 *   l  = rot((-quat'.x, -quat'.y, -quat'.z), quat'.w, r)
 *   dp = sqrtf((r.x*r.x + r.y*r.y) + r.z*r.z)
 *   unless l.z > 0: NOHIST
 *   sx = ((((l.x * cam'.focal) / l.z) + cam'.viewport[0]*0.5f) * view_w) / cam'.viewport[0]
 *   sy = ((((l.y * cam'.focal) / l.z) + cam'.viewport[1]*0.5f) * view_h) / cam'.viewport[1]
 *   u = sx - (float)x0;  v = sy - (float)y0
 *   unless u >= -1.0f && u < (float)w && v >= -1.0f && v < (float)h: NOHIST     (a NaN fails)
 *   fu = floorf(u); a = u - fu; i0 = (int)fu;   fv = floorf(v); b = v - fv; j0 = (int)fv
 *   S = (0,0,0); SN = 0; W = 0
 *   for (dx,dy) in (0,0), (1,0), (0,1), (1,1):
 *     q = (i0+dx, j0+dy); skip q outside [0,w) x [0,h)
 *     skip unless id'_q == id_p (all 32 bits)  and  al'_q.w == al_p.w
 *            and (nd_p.x*nd'_q.x + nd_p.y*nd'_q.y) + nd_p.z*nd'_q.z >= 0
 *            and fabsf(dp - nd'_q.w) <= tol_z * (dp + nd'_q.w)
 *     g = (dx ? a : 1.0f - a) * (dy ? b : 1.0f - b)
 *     S.c = S.c + g * H'_q.c  (c = r, g, b);  SN = SN + g * H'_q.a;  W = W + g
 *   unless W >= w_min: NOHIST
 *   Hc = S / W;  N = fminf(SN / W + 1.0f, (float)n_max)
 *   out.rgb = Hc + (C.rgb - Hc) / N;  out.a = N
 *
 * MM_ERR_INVALID: a null argument other than prev, a null pointer in guides or
 * in prev (its colour, its guides); n_max outside 1..65535, tol_z not > 0 or
 * not finite, w_min outside (0, 1] (a NaN is outside), flags not 0; w, h or
 * n_frames 0; a misaligned pointer (float4: 16 bytes, id: 4); out_dev
 * overlapping color_dev, a guide or a prev buffer (prev may be an earlier
 * call's out_dev, not this one's); w*h over 2^31 - 1, x0 + w or y0 + h over
 * 2^24 (the float conversions are then exact), or more than 2^40 pixels in
 * all.  Enqueued on the context's stream like mm_denoise_frames, one launch per
 * frame in stream order; the inputs are never written.  The call keeps no
 * scratch (frame f reads frame f-1 from out_dev) and needs no uploaded scene. */
int  mm_accumulate_frames(mm_ctx* ctx, const mm_uniform* uni, const mm_camera* cams,
                          const float* color_dev, const mm_aov* guides,
                          const mm_temporal_prev* prev, const mm_temporal_params* p,
                          uint32_t n_frames, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                          void* out_dev);

/* ---- a pixel list, and topping up short histories ------------------------------
 * mm_trace_pixels traces a caller-supplied SET of pixels of the frame, one
 * launch (plus the resolve launch when the samples are staged), one camera
 * (uni->cam), one frame: region-of-interest re-renders, progressive
 * refinement, a few pixels of a large frame against an oracle, and extra
 * samples for the pixels whose history mm_accumulate_frames left short.
 *
 * pixels_dev: DEVICE pointer, 8-byte aligned, n_pixels pairs (x, y) of uint32
 * in view coordinates; stream-ordered -- the caller keeps it unchanged until
 * the call has finished, the context makes no copy.  out_dev: n_pixels float4
 * (16-byte aligned), or 4-byte RGBA8 pixels with MM_EXT_RGBA8; element e
 * belongs to list entry e.  For an entry inside the view out[e] equals, on all
 * bits, pixel (x, y) of mm_trace_tile with the same uni and ext: the same
 * primary direction, RNG stream (pixel y*view_w + x, sample, ext->frame),
 * bounce loop and summation order, for any spp in 1..4096.  MM_EXT_RGBA8: the
 * texture-write conversion of that float4; MM_EXT_ACCUMULATE: out[e] += the
 * value, alpha += 1; MM_EXT_COUNT_STATS fills stats as mm_trace_tile does
 * (rays and paths exact).  The list's order is free; a pixel may appear more
 * than once, and each entry gets its own, equal, result (with
 * MM_EXT_ACCUMULATE each entry accumulates into its own element).  An entry
 * with x >= view_w or y >= view_h is not traced: it writes (0, 0, 0, 0)
 * (RGBA8: 0) or, with MM_EXT_ACCUMULATE, nothing, counts in neither paths nor
 * rays, and is not an error.
 *
 * n_pixels = 0: MM_OK, nothing enqueued, no call number taken.  MM_ERR_INVALID:
 * a null argument, a misaligned pointer, spp or the limits out of range (as in
 * mm_trace_tile), MM_EXT_RGBA8 with MM_EXT_ACCUMULATE, n_pixels * spp (in
 * chunks padded to 64) beyond the launch's 32-bit queue, or beyond the 2^29
 * staged paths when the samples are staged (64 % spp != 0, MM_OPT_FUSE_RESOLVE
 * 0 or MM_PIPE_REFERENCE).  MM_ERR_NO_SCENE without a scene; an earlier failed
 * call is reported first.  Enqueued on the context's stream and numbered like
 * the tile calls.  The launch never runs the mirror-tail rings (MM_OPT_DEFER
 * and MM_OPT_DEFER_MIN select nothing, MM_INFO_LAST_DEFER reads 0 after it;
 * MM_PIPE_WAVEFRONT: MM_ERR_UNSUPPORTED); MM_PIPE_REFERENCE is supported. */
int  mm_trace_pixels(mm_ctx* ctx, const mm_uniform* uni, const mm_ext* ext,
                     const uint32_t* pixels_dev, uint64_t n_pixels,
                     void* out_dev, mm_stats* stats);

/* Extra samples into an accumulated frame, in place.  image_dev: w*h float4
 * (16-byte aligned), the window (x0, y0, w, h) with y_stride 1 whose alpha is
 * the history length N as mm_accumulate_frames writes it.  pixels_dev: the
 * list (as above); extra_dev: n_pixels float4 (16-byte aligned), an
 * mm_trace_pixels output for the same list.  m: the weight of the extra
 * samples in frames (extra spp / frame spp), finite and > 0.
 *
 * All arithmetic is IEEE binary32, no contraction, in the order written; / is
 * correctly rounded.  For entry e, (x, y) = pixels[e]:
 *   skip the entry unless x0 <= x < x0 + w and y0 <= y < y0 + h
 *   p = (y - y0)*w + (x - x0);  A = image[p];  E = extra[e];  Nn = A.a + m
 *   image[p].c = A.c + ((E.c - A.c) * m) / Nn  (c = r, g, b);  image[p].a = Nn
 * A list that names a window pixel twice leaves that pixel with one of the two
 * results, unspecified which.
 *
 * MM_ERR_INVALID: a null context, image, list or extra_dev; a misaligned
 * pointer; w or h 0, or w*h over 2^31 - 1; m not finite or not > 0; extra_dev
 * overlapping image_dev.  n_pixels = 0: MM_OK.  Enqueued on the context's
 * stream like mm_accumulate_frames; needs no uploaded scene. */
int  mm_blend_pixels(mm_ctx* ctx, float* image_dev, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                     const uint32_t* pixels_dev, const float* extra_dev, uint64_t n_pixels, float m);

/* ---- per-pixel sample variance -------------------------------------------------
 * The trace calls return each pixel's sample mean.  These two return, beside
 * it, the sample variance of the pixel's luminance: how noisy the pixel is,
 * for sampling where the noise is (Renderer.refine), for a stopping rule, and
 * for a variance-guided filter.  The variance is taken where the samples
 * already are: the calls always stage the samples (the path MM_OPT_FUSE_RESOLVE
 * 0 takes, also at spp the plain calls would resolve in the wave), and the
 * resolve that reads them for the mean takes their second moment with it.
 *
 * mm_trace_tile_var: out_dev is, on all bits, what the plain call writes for
 * the same arguments -- mm_trace_tile for cams == NULL and n_frames == 1,
 * mm_trace_tile_frames for cams == NULL, mm_trace_tile_cameras for cams !=
 * NULL (a HOST array of n_frames cameras, consumed on return).
 * mm_trace_pixels_var: out_dev is what mm_trace_pixels writes.  MM_EXT_RGBA8
 * is allowed (out_dev then holds 4-byte pixels; var_dev does not change).
 * var_dev: DEVICE pointer, 4-byte aligned, one float per pixel or list entry
 * at out_dev's element index: f*w*h + j*w + i for a tile, e for a list.
 *
 * All arithmetic is IEEE binary32, no contraction, in the order written; / is
 * correctly rounded.  s_0 .. s_{spp-1} are the pixel's samples, the ones the
 * mean is taken of;
 *   T(x) = the resolve's summation order: spp % 8 == 0: blocks of 8 summed as
 *          ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)), the blocks added left to
 *          right; otherwise x0 + x1 + ... left to right
 *   l_k  = (0.25f*s_k.r + 0.5f*s_k.g) + 0.25f*s_k.b     (mm_denoise_frames' lum)
 *   ml   = T(l) / (float)spp
 *   q_k  = (l_k - ml) * (l_k - ml)
 *   var  = T(q) / (float)(spp - 1)
 * var is the unbiased sample variance of ONE sample's luminance; var / spp
 * estimates the variance of the pixel's mean.  (Two passes over samples that
 * lie in memory: no one-pass form and its cancellation.)  A list entry outside
 * the view writes var = 0 (and out as mm_trace_pixels does).
 *
 * Every condition of the plain call with MM_OPT_FUSE_RESOLVE 0 applies: the
 * 2^29 staged paths of a list or a multi-frame launch (a single frame beyond
 * the staging bound is traced in row batches), the 2^32 queue, and a multi-frame
 * launch needs tail deferral (it reports the plain call's error where the
 * plan has none).  MM_ERR_INVALID in addition: spp < 2, MM_EXT_ACCUMULATE, a
 * null or misaligned var_dev, var_dev overlapping out_dev.  n_pixels = 0:
 * MM_OK, nothing enqueued.  Enqueued and numbered like the plain calls; the
 * call tracker names them mm_trace_tile_var and mm_trace_pixels_var, and
 * mm_last_timing counts two launches per row batch. */
int  mm_trace_tile_var(mm_ctx* ctx, const mm_uniform* uni, const mm_camera* cams,
                       const mm_ext* ext, uint32_t n_frames,
                       uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride,
                       void* out_dev, float* var_dev, mm_stats* stats);
int  mm_trace_pixels_var(mm_ctx* ctx, const mm_uniform* uni, const mm_ext* ext,
                         const uint32_t* pixels_dev, uint64_t n_pixels,
                         void* out_dev, float* var_dev, mm_stats* stats);

/* ---- pixel lists of many frames in one launch -----------------------------------
 * mm_trace_pixel_lists traces n_lists pixel lists, each with its own camera and
 * RNG frame, in ONE launch (plus the resolve launch when the samples are
 * staged): the refinement lists of a batch of frames, which have no dependency
 * on each other, without one small launch per frame.
 *
 * pixels_dev: DEVICE pointer, 8-byte aligned, offsets[n_lists] pairs (x, y):
 * the lists back to back; stream-ordered and not copied, as in mm_trace_pixels.
 * offsets: HOST array of n_lists + 1 values, offsets[0] == 0, non-decreasing;
 * list f is entries offsets[f] .. offsets[f+1] - 1 and may be empty.  cams:
 * HOST array of n_lists cameras, or NULL for uni->cam on every list;
 * frame_keys: HOST array of n_lists RNG frames, or NULL for ext->frame + f.
 * The three host arrays are consumed on return.  out_dev: offsets[n_lists]
 * float4 (or 4-byte pixels with MM_EXT_RGBA8); element e belongs to global
 * entry e.
 *
 * var_dev == NULL: entry e of list f equals, on all bits, what mm_trace_pixels
 * writes for it with uni->cam = cams[f] and ext->frame = frame_keys[f], under
 * every rule of that call (entries outside the view, duplicates,
 * MM_EXT_ACCUMULATE, MM_EXT_RGBA8, any spp in 1..4096; the resolve is fused
 * or the samples staged by the same rule).  var_dev != NULL: offsets[n_lists]
 * floats, 4-byte aligned, not overlapping out_dev; (out, var) are
 * mm_trace_pixels_var's per entry, bit for bit, under that call's conditions
 * (spp >= 2, no MM_EXT_ACCUMULATE, samples always staged).  stats: summed over
 * the lists (rays and paths exact).
 *
 * A total of 0 entries: MM_OK, nothing enqueued, no call number taken.
 * MM_ERR_INVALID: n_lists outside 1..65535; a null offsets, offsets[0] != 0 or
 * a decreasing offset; with entries to trace, a null uni, ext, pixels_dev or
 * out_dev, a misaligned pointer, MM_EXT_RGBA8 with MM_EXT_ACCUMULATE, spp or
 * the limits out of range; the queue -- the sum over the lists of n_f * spp
 * padded to 64, so that every list starts on a chunk boundary -- beyond the
 * launch's 32-bit counter; more than 2^29 staged paths when the samples are
 * staged.  MM_ERR_NO_SCENE without a scene; an earlier failed call is reported
 * first.  MM_PIPE_WAVEFRONT: MM_ERR_UNSUPPORTED.  MM_PIPE_REFERENCE runs one
 * reference list launch per non-empty list under the one call number (a
 * baseline, not a rate).  Otherwise one wave-persistent launch, plus one
 * resolve launch when the samples are staged (mm_last_timing counts 1 or 2);
 * the launch never runs the mirror-tail rings (MM_INFO_LAST_DEFER reads 0).
 * Numbered like the other trace calls; the call tracker names it
 * mm_trace_pixel_lists with n_lists, the entries and spp.  The per-list records
 * are context-owned and staged on the stream ahead of the launch, as
 * mm_trace_tile_cameras stages cameras: back-to-back calls never share records
 * and never wait on the host. */
int  mm_trace_pixel_lists(mm_ctx* ctx, const mm_uniform* uni, const mm_camera* cams,
                          const mm_ext* ext, const uint32_t* frame_keys, uint32_t n_lists,
                          const uint32_t* pixels_dev, const uint64_t* offsets,
                          void* out_dev, float* var_dev, mm_stats* stats);

/* ---- radiance along caller-supplied rays ------------------------------------------
 * The trace calls above start every path at uni->cam.center along a pinhole
 * camera's primary direction; mm_query_rays takes any ray but returns only its
 * first hit.  mm_trace_rays answers "what radiance arrives along this ray":
 * the shaded, averaged value of the path statement for each ray of a list, in
 * one launch (plus the resolve launch when the samples are staged) -- other
 * cameras (equirectangular, orthographic, fisheye, stereo), light probes,
 * radiance leaving a point of a wall, one path replayed for debugging.  There
 * is no uni: no camera and no view.
 *
 * rays_dev: DEVICE pointer, 16-byte aligned, 8 words per ray:
 * (ox, oy, oz, key, dx, dy, dz, -), mm_query_rays' record.  Word 3 is read as
 * a uint32_t RNG key (its bit pattern, not a float conversion); word 7 is
 * ignored.  Stream-ordered -- the caller keeps the buffer unchanged until the
 * call has finished, the context makes no copy.  Any ray mm_query_rays allows
 * is allowed: origins outside the scene or on a wall, unnormalised directions,
 * zero components.  ray_flags: 0 or MM_RAYS_JITTER.
 *
 * Sample s (0 .. spp-1) of entry e runs the path statement of
 * src/shaders.metal:302-344 (the bounce loop every trace call runs) with
 *   ori  = (ox, oy, oz)
 *   seed = the throughput-mode seed of (pixel = key, sample = s, ext->frame),
 *          the function mm_trace_tile applies to pixel y*view_w + x
 *   dir  = (dx, dy, dz) as given, no random number drawn before the first
 *          bounce; with MM_RAYS_JITTER, d + (j1*0.001f, j2*0.001f, 0.0f*0.001f)
 *          where j1, j2 are the seed's first two draws: the primary ray's
 *          jitter exactly (a dz of -0.0f becomes +0.0f, as -0.0f + 0.0f is)
 * and ext->bounce_limit / ext->mirror_limit.  The sample's value is
 * sqrt(max(L, 0)) as in every trace call.
 *
 * out_dev: n_rays float4 (16-byte aligned), or 4-byte RGBA8 pixels with
 * MM_EXT_RGBA8.  out[e] is the mean of entry e's spp sample values in the
 * resolve's order T (mm_trace_tile_var above), divided by (float)spp, alpha 1:
 * what mm_trace_tile defines for a pixel.  MM_EXT_RGBA8, MM_EXT_ACCUMULATE and
 * MM_EXT_COUNT_STATS behave exactly as in mm_trace_pixels (stats: rays and
 * paths exact).  Duplicate records get equal results, each in its own element.
 * var_dev: NULL, or n_rays floats (4-byte aligned, not overlapping out_dev):
 * mm_trace_pixels_var's variance per entry under that call's conditions
 * (spp >= 2, no MM_EXT_ACCUMULATE, the samples always staged); out is the same
 * with and without it.
 *
 * Equivalence: with MM_RAYS_JITTER and, for each pixel (x, y) of a list, the
 * record (uni->cam.center, y*view_w + x, primary direction of (x, y) under
 * uni), out equals mm_trace_pixels' -- and var mm_trace_pixels_var's -- for
 * the pixel list (x, y) on all bits.
 *
 * n_rays = 0: MM_OK, nothing enqueued, no call number taken.  MM_ERR_INVALID,
 * the first that applies: a null ext, rays_dev or out_dev; a misaligned
 * rays_dev or out_dev; unknown ray_flags; spp or the limits out of range (as
 * in mm_trace_tile); MM_EXT_RGBA8 with MM_EXT_ACCUMULATE; with var_dev, that
 * call's conditions (spp < 2, MM_EXT_ACCUMULATE, a misaligned var_dev, var_dev
 * overlapping out_dev); n_rays * spp (in chunks padded to 64) beyond the
 * launch's 32-bit queue; more than 2^29 staged paths when the samples are
 * staged (64 % spp != 0, MM_OPT_FUSE_RESOLVE 0, MM_PIPE_REFERENCE or var_dev);
 * a null context.  MM_ERR_NO_SCENE without a scene; an earlier failed call is
 * reported first.  MM_PIPE_WAVEFRONT: MM_ERR_UNSUPPORTED (the launch never
 * runs the mirror-tail rings: MM_OPT_DEFER and MM_OPT_DEFER_MIN select nothing
 * and MM_INFO_LAST_DEFER reads 0 after it); MM_PIPE_REFERENCE runs the
 * one-thread-per-path kernel.  A traversal-stack overflow is reported as
 * MM_ERR_STACK, as in the tile calls.  Enqueued on the context's stream,
 * numbered and timed like the other trace calls (mm_last_timing counts 1 or 2
 * launches); the call tracker names it mm_trace_rays with the ray count and
 * spp. */
#define MM_RAYS_JITTER 0x1u
int  mm_trace_rays(mm_ctx* ctx, const mm_ext* ext, uint32_t ray_flags,
                   const float* rays_dev, uint64_t n_rays,
                   void* out_dev, float* var_dev, mm_stats* stats);

/* ---- variance through the history ----------------------------------------------
 * mm_accumulate_frames with the variance of the pixel mean carried beside the
 * colour, and a weight per pixel and frame: the accumulated frame then has
 * what mm_denoise_frames_var (vmean = var_out) and a noise-driven top-up ask
 * for, and frames with unequal sample counts (Renderer.refine) accumulate.
 *
 * Everything mm_accumulate_frames states holds: uni, cams, color_dev, guides,
 * p, the window, the projection, the four taps, the key test, w_min, IEEE
 * binary32 in the order written with no contraction, subnormals kept, / and
 * sqrtf correctly rounded.  vmean_dev: n_frames*w*h floats (4-byte aligned),
 * the variance of the frame's pixel-MEAN luminance (mm_trace_tile_var's var /
 * the pixel's sample count).  weight_dev: n_frames*w*h floats or NULL, the
 * frame's weight m per pixel in frames (samples held / frame spp, e.g. after
 * Renderer.refine); NULL: 1 everywhere.  prev: as mm_temporal_prev, and var,
 * that frame's var_out of the earlier call.  out_dev: n_frames*w*h float4,
 * out.a is the history length N in frames (a float >= the least weight);
 * var_out_dev: n_frames*w*h floats, the variance of out's luminance.  The
 * call is defined for finite m > 0 and finite V >= 0.  Frame f reads frame
 * f-1's colour AND variance from this call's own outputs; for f = 0 it reads
 * prev, or none if prev is NULL.  V' is the history frame's variance output.
 * For pixel p of frame f:
 *   m  = weight ? weight[f][p] : 1.0f;  Vc = vmean[f][p]
 *   NOHIST: out = (C.r, C.g, C.b, m);  Vout = Vc
 *   SV = 0; in the tap loop, for every tap that is not skipped, after W = W + g:
 *     SV = SV + (g * g) * V'_q
 *   unless W >= w_min: NOHIST
 *   Hc = S / W;  VH = SV / (W * W)
 *   N  = fminf(SN / W + m, fmaxf((float)n_max, m))          (m / N never exceeds 1)
 *   out.c = Hc.c + ((C.c - Hc.c) * m) / N  (c = r, g, b);  out.a = N
 *   b = m / N;  c = 1.0f - b
 *   Vout = (c * c) * VH + (b * b) * Vc
 * With weight_dev == NULL out_dev equals mm_accumulate_frames' output for the
 * same arguments on all bits: (C - Hc) * 1.0f is exact, fmaxf(n_max, 1) is
 * n_max, and NOHIST writes alpha 1.0f.
 *
 * VH weights the taps' variances by g*g, the form mm_denoise_frames_var uses:
 * it takes the taps as independent.  Neighbouring history pixels share
 * ancestors once a frame has been reprojected between pixel centres, so Vout
 * falls short of the true variance of out (a desk model of iid noise under
 * repeated bilinear reprojection, scripts/temporal_var_model.py: 0.78..1.00 of
 * it over 8 frames; the linear form sum g V' / W gives 1.0..4.7); DESIGN.md s4
 * "Variance through the history" has what was measured on rendered frames.
 *
 * MM_ERR_INVALID: everything mm_accumulate_frames rejects; a null vmean_dev or
 * var_out_dev; prev with a null var; a vmean_dev, weight_dev, var_out_dev or
 * prev->var that is not 4-byte aligned; out_dev or var_out_dev overlapping any
 * input, a prev buffer, or each other.  None of the checks needs the context;
 * a null context is refused last.  Enqueued on the context's stream, one
 * launch per frame in stream order; the inputs are never written; the call
 * keeps no scratch and needs no uploaded scene. */
int  mm_accumulate_frames_var(mm_ctx* ctx, const mm_uniform* uni, const mm_camera* cams,
                              const float* color_dev, const mm_aov* guides,
                              const float* vmean_dev, const float* weight_dev,
                              const mm_temporal_prev_var* prev, const mm_temporal_params* p,
                              uint32_t n_frames, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                              void* out_dev, float* var_out_dev);

/* mm_blend_pixels with the variance image beside the colour, both in place.
 * image_dev, the window, pixels_dev, extra_dev, n_pixels, m: as mm_blend_pixels.
 * var_dev: w*h floats (4-byte aligned), the window's var_out of
 * mm_accumulate_frames_var; extra_vmean_dev: n_pixels floats (4-byte aligned),
 * the variance of the extra samples' MEAN (mm_trace_pixels_var's var / extra
 * spp).  The colour and alpha are exactly mm_blend_pixels'; in addition, for an
 * entry that is not skipped, with Nn = A.a + m as there:
 *   b = m / Nn;  c = 1.0f - b
 *   var[p] = (c * c) * var[p] + (b * b) * extra_vmean[e]
 * The skip rule, the duplicate rule and n_pixels = 0 are mm_blend_pixels'.
 * MM_ERR_INVALID: everything mm_blend_pixels rejects; a null or misaligned
 * var_dev or extra_vmean_dev; var_dev overlapping image_dev, the list,
 * extra_dev or extra_vmean_dev; the list or extra_vmean_dev overlapping
 * image_dev. */
int  mm_blend_pixels_var(mm_ctx* ctx, float* image_dev, float* var_dev,
                         uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const uint32_t* pixels_dev,
                         const float* extra_dev, const float* extra_vmean_dev, uint64_t n_pixels, float m);

/* Frames traced on a pixel lattice, rebuilt at full resolution from the AOVs.
 *
 * primary_dir maps pixel px to the screen point vx*px/view_w - vx/2, with no
 * half-pixel offset, so for s a power of two pixel (X, Y) of the view
 * (view_w/s, view_h/s) looks along the direction of pixel (sX, sY) of the full
 * view, bit for bit: a frame traced at 1/s of the view IS the full frame's
 * lattice of every s-th pixel, and the full-resolution guides at the lattice
 * pixels are its guides.  This call interpolates the lattice's colours to every
 * pixel of the window, across one surface only (also a surface seen in a
 * mirror), and marks the pixels no lattice neighbour can stand in for: holes,
 * which mm_trace_pixel_lists and mm_fill_pixels then fill.
 *
 * s = p->scale; lw = ceil(w/s), lh = ceil(h/s).  low_dev: n_frames*lw*lh float4,
 * frame-major; element (X, Y) is the traced value of window pixel (sX, sY) --
 * mm_trace_tile / _frames / _cameras / _var with the view (view_w/s, view_h/s)
 * and the tile (x0/s, y0/s, lw, lh), where x0, y0 and the view size are
 * multiples of s.  The call itself works in window index space, as
 * mm_denoise_frames does.  guides: the three full-resolution buffers of one
 * mm_trace_aov call over (w, h), all required.  low_vmean_dev: n_frames*lw*lh
 * floats, the variance of the lattice pixels' MEAN luminance, or NULL (then
 * var_out_dev must be NULL); given without var_out_dev it is checked and not
 * read.  out_dev: n_frames*w*h float4; weight_out_dev and
 * var_out_dev: n_frames*w*h floats, or NULL.
 *
 * All arithmetic is IEEE binary32, no contraction, in the order written;
 * subnormals are kept and / is correctly rounded.  L is low_dev, VL
 * low_vmean_dev, nd / al / id the guides.  For pixel p = (x, y) of frame f:
 *   X0 = x / s; Y0 = y / s                                   (integers)
 *   a = (float)(x - s*X0) * (1.0f / (float)s);  b = (float)(y - s*Y0) * (1.0f / (float)s)
 *   HOLE: out = (0,0,0,0); weight = 0; var = 0
 *   if id_p == MM_AOV_ID_FAILED: HOLE
 *   S = (0,0,0); W = 0; G2 = 0; SV = 0
 *   for (dx,dy) in (0,0), (1,0), (0,1), (1,1):
 *     Q = (X0+dx, Y0+dy); skip Q outside [0,lw) x [0,lh)
 *     g = (dx ? a : 1.0f - a) * (dy ? b : 1.0f - b); skip unless g > 0
 *     q = window pixel (s*Q.x, s*Q.y)
 *     skip unless id_q == id_p (all 32 bits) and al_q.w == al_p.w
 *            and (nd_p.x*nd_q.x + nd_p.y*nd_q.y) + nd_p.z*nd_q.z >= 0
 *     S.c = S.c + g * L_Q.c (c = r,g,b);  W = W + g;  G2 = G2 + g*g;  SV = SV + (g*g) * VL_Q
 *   unless W >= w_min: HOLE
 *   out = (S.r / W, S.g / W, S.b / W, 1.0f);  weight = (W*W) / G2;  var = SV / (W*W)
 * There is no depth term: one planar rect seen through the same mirrors from
 * the same side is the whole test (a soft depth term made more holes and a
 * worse frame, DESIGN.md s4 "Tracing a lattice and rebuilding from the AOVs").
 * A lattice pixel has one tap with g = 1: it returns its traced value, its
 * variance and weight 1 on all bits.  weight is the pixel's effective sample
 * weight in frames, in [1, 4], what mm_accumulate_frames_var takes as
 * weight_dev once the holes are filled; 0 marks a hole.  var is EXACT for the
 * noise part: the taps are distinct lattice pixels with independent samples
 * (unlike mm_denoise_frames_var's Vout and mm_accumulate_frames_var's, whose
 * taps share ancestors); what it leaves out is the interpolation's own error.
 *
 * MM_ERR_INVALID, in this order: a null low_dev, guides, p or out_dev, or a
 * null guide buffer; scale not 2, 4 or 8; w_min outside (0, 1] (a NaN counts
 * as outside); flags or reserved not 0; w, h or n_frames 0; a pointer that is
 * not aligned (float4: 16 bytes; id, variances and weights: 4); var_out_dev
 * given without low_vmean_dev; w*h above 2^31 - 1, n_frames*w*h above 2^40 or
 * n_frames * ceil(w/64) * ceil(h/4) above 2^26 - 1 (one launch's blocks); an
 * output overlapping an input; two outputs overlapping.  None of the checks
 * needs the context; a null context is refused last.  Enqueued on the
 * context's stream, ONE launch for all frames; the inputs are never written;
 * the call keeps no scratch and needs no uploaded scene. */
int  mm_upsample_frames(mm_ctx* ctx, const float* low_dev, const mm_aov* guides,
                        const float* low_vmean_dev, const mm_upsample_params* p,
                        uint32_t n_frames, uint32_t w, uint32_t h,
                        void* out_dev, float* weight_out_dev, float* var_out_dev);

/* Replace the pixels of a list in a window's images, in place: what fills
 * mm_upsample_frames' holes with traced pixels.  image_dev, the window,
 * pixels_dev, extra_dev, n_pixels: as mm_blend_pixels_var; var_dev and
 * weight_dev: w*h floats each (4-byte aligned), or NULL; extra_vmean_dev:
 * n_pixels floats, given exactly when var_dev is.  For an entry e inside the
 * window, at pixel p:
 *   image[p] = extra[e]  (all four floats);  var[p] = extra_vmean[e];  weight[p] = m
 * each where its buffer is given: copies, exact on all bits.  (mm_blend_pixels
 * cannot do this: with A.a = 0 it computes (E*m)/m, which is not E on all
 * bits.)  The skip rule, the duplicate rule and n_pixels = 0 are
 * mm_blend_pixels': entries outside the window touch nothing, the list must
 * not name a window pixel twice, and an empty list returns MM_OK without a
 * look at the list's buffers.
 * MM_ERR_INVALID, in this order: a null image_dev; an empty window or more
 * than 2^31 - 1 pixels; m not positive and finite; a misaligned image_dev,
 * var_dev or weight_dev; two of those overlapping; then, for n_pixels > 0: a
 * null pixels_dev or extra_dev; var_dev without extra_vmean_dev or the
 * reverse; a misaligned list buffer (float4: 16 bytes, the list: 8,
 * variances: 4); n_pixels above 2^38; a list buffer overlapping image_dev,
 * var_dev or weight_dev.  A null context is refused last. */
int  mm_fill_pixels(mm_ctx* ctx, float* image_dev, float* var_dev, float* weight_dev,
                    uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                    const uint32_t* pixels_dev, const float* extra_dev,
                    const float* extra_vmean_dev, uint64_t n_pixels, float m);

/* Pipeline selection for mm_trace_tile (MM_PIPE_AUTO picks the fastest). */
#define MM_PIPE_AUTO       0
#define MM_PIPE_MEGAKERNEL 1   /* bounce loop in-kernel (MM_OPT_PERSIST picks the kernel) */
#define MM_PIPE_WAVEFRONT  2   /* the wave-persistent kernel with the mirror-tail deferral always on
                                  (MM_OPT_DEFER, 32 lanes unless set): a wave's divergent tail is parked
                                  in its block's ring and resumed 64 paths at a time, densely.  The round-1
                                  fully flattened pipeline
                                  (SoA state in HBM, one extend/shade launch pair per bounce) measured
                                  ~45 ms vs 5.7 ms per C3 frame and was retired (DESIGN.md §4,
                                  profiles/r02/wavefront_pmc.txt) */
#define MM_PIPE_REFERENCE  3   /* straight statement of the reference kernel, one thread per path
                                  (IEEE division everywhere); A/B baseline  */
int  mm_set_pipeline(mm_ctx* ctx, int pipe);

/* Tuning knobs (results never change; only speed does).  Every value is
 * bit-identical to the reference; the defaults are the measured fastest
 * (DESIGN.md §4).  Options removed after round 1 (measured slower or
 * neutral: 4, 5, 6, 10, 11, 13-17) return MM_ERR_INVALID. */
#define MM_OPT_LDS_NODES   1   /* 1: stage scene data (BVH or grid) in LDS where it fits (default), 0: read
                                  everything through L1/L2 */
#define MM_OPT_BLOCK       2   /* threads per workgroup of MM_PIPE_REFERENCE's one-thread-per-path kernel
                                  (64..1024, x64) */
#define MM_OPT_PERSIST     3   /* 2: wave-persistent kernel, 64-path chunks, pixels resolved in the wave
                                  (default, the only one); 0 (one thread per path) was removed in round 6:
                                  MM_ERR_UNSUPPORTED */
#define MM_OPT_TRAVERSAL   7   /* closest-hit query of the wave-persistent kernel:
                                  -1 auto (default): 11 when the scene allows it, else 7 when every rect has a
                                     compact record, else 5;
                                  11 certified grid search (mm_grid.h): same answer as the reference's BVH walk,
                                     which runs instead on ties / failed certificates / rays outside the grid;
                                  0 (the reference's BVH loop form) was removed in round 6: MM_ERR_UNSUPPORTED
                                    (the parity-mode kernel, mm_trace_chunks, still walks it);
                                  5 BVH, leaf tests and the next interior step in one iteration;
                                  7 form 5 with branch-free compact leaf tests (scenes without SLOW records) */
#define MM_OPT_LDS_RECTS   8   /* BVH forms: 1 compact rect records in LDS beside the nodes when both fit (default) */
#define MM_OPT_LDS_SPLIT   9   /* removed in round 6 (the top-of-tree node cache measured slower): 0 / 1 are
                                  accepted and select nothing, > 1 returns MM_ERR_UNSUPPORTED */
#define MM_OPT_FUSE_RESOLVE 12 /* wave-persistent kernel: 1 reduce each pixel's samples inside the wave
                                  that traced them when 64 % spp == 0 (default), 0 separate k_resolve */
#define MM_OPT_RESERVE_CUS 19 /* wave-persistent kernel: launch that many CUs' worth of resident blocks
                                  fewer (0..128), so kernels of other streams -- a collective moving the
                                  previous frames -- find free CUs while it runs; 0 default */
#define MM_OPT_DICT_NODES 20  /* removed in round 6 (dictionary-coded BVH nodes measured slower): 0 / 1 are
                                  accepted and select nothing, 2 returns MM_ERR_UNSUPPORTED */
#define MM_OPT_DEFER      21  /* wave-persistent kernel: once at most this many lanes of a wave still trace
                                  (past bounce_limit only mirror-hit paths run on), those paths' states go to
                                  their block's tail ring (512 entries) and the block's waves take 64 of them at
                                  a time as a chunk of their own; samples are then staged per path and resolved
                                  by k_resolve (same order).  0 off, 1..64; default: 32 when the search
                                  structure sits whole in LDS (the maze grid with its leaf boxes, or BVH nodes +
                                  compact records) and bounce_limit >= 8 (C3, 20 frames per launch: 2.64 ms/frame
                                  on vs 2.74 off; C4 20.97 vs 21.80), or 64 % spp != 0 (samples staged anyway),
                                  else off (the N=64 scene, leaf boxes via L1/L2: 5.23 on vs 4.90 off) --
                                  profiles/r03/ab_defer_claims.txt.  Built for the grid search and the lean BVH
                                  form with records in LDS; other forms ignore it */
#define MM_OPT_DEFER_MIN  22  /* MM_OPT_DEFER applies to launches of at least this many paths (w*h*spp*frames;
                                  default 2^24: a single C3 frame (16.6 M paths) runs without the rings; rank
                                  0 of an 8-way C3 split, 20 frames = 41 M paths per launch, 0.356 ms/frame
                                  with them vs 0.362 without -- profiles/r03/emulated_scaling/); 0: always */
#define MM_OPT_GRID_MERGE 24  /* grid search: 1 (default) an axis whose cells would not shorten the lists
                                  gets one cell (the maze: one cell along y -- its walls span the height, the
                                  lower cell is the space below the floor); 0 cells per axis by the typical
                                  rect size only.  Read by mm_upload_scene */
#define MM_OPT_GRID_CELL  25  /* grid search: the first cell size tried, in percent of the median rect extent
                                  (25..400, default 100; coarser cells follow until the index fits the LDS
                                  budget).  Read by mm_upload_scene */
#define MM_OPT_GRID_WIDE  26  /* grid search: 1 (default) 64-bit cell words with per-face list ranges where the
                                  image fits the LDS budget; 0 plain 32-bit words (whole list per cell).  Read
                                  by mm_upload_scene */
#define MM_OPT_PREDRAW    27  /* wave-persistent kernel: rejection-sampling trials a chunk of new paths draws
                                  per path before its bounces, acceptance only, into the path's trial window
                                  from its own stream (the pre-pass's own rounds; 0..31; -1 default: with
                                  MM_OPT_PREDRAW_POOL 2 * (bounce_limit - 1) -- 14 at 8 bounces -- up to 24, else
                                  3 * bounce_limit, at most 31; scripts/predraw_model.py,
                                  scripts/predraw_pool_model.py, profiles/predraw/, profiles/pool/).  Results
                                  never depend on it */
#define MM_OPT_PREDRAW_POOL 28 /* wave-persistent kernel: 1 (default) after the own rounds the wave's lanes draw,
                                  pooled, the further trials of the paths whose windows hold fewer accepted
                                  trials than the path reads (cross-lane permutes; mm_trace.h pool_trials);
                                  0 own rounds only.  Results never depend on it */
#define MM_OPT_UPSAMPLE_LDS 29 /* mm_upsample_frames: 1 (default) a block stages its lattice footprint (at most
                                  33 x 3 pixels) in LDS and the taps read it there; 0 the taps gather the
                                  lattice from global memory.  The same arithmetic on the same values; staging
                                  measured 0.78 (scale 2) and 0.87 (scale 4) of the gathers' time
                                  (profiles/upsample/ab.txt) */
#define MM_OPT_FAULT_INJECT 23 /* tests of the error path (results are then invalid): 0 off (default); 1 every
                                  wave-persistent launch raises an injected fault (error bit 3); 2 the tail
                                  rings' protocol waits give up at once (bit 2 when a wait was needed; a
                                  writer that gives up leaves NaN in its sample, mm_last_error names the
                                  first timed-out wait); 3 the trace call fails with MM_ERR_HIP after
                                  taking its first launch's status slot, before the launch is enqueued;
                                  4 the launch's first deferred path is lost (its ring entry is reserved,
                                  never written): its reader times out after the normal bound and every
                                  later protocol wait of the launch gives up within 256 polls */
/* The library holds the kernels MM_PIPE_AUTO can select; the values that chose
 * the variants removed in round 6 (MM_OPT_PERSIST 0, MM_OPT_TRAVERSAL 0,
 * MM_OPT_LDS_SPLIT > 1, MM_OPT_DICT_NODES 2, BVH form 7 without nodes +
 * records in LDS) return MM_ERR_UNSUPPORTED. */
int  mm_set_option(mm_ctx* ctx, int key, int value);

/* Facts about the uploaded scene's search structures (double-valued):
 *   MM_INFO_GRID_OK          1 if the certified grid search is available
 *   MM_INFO_GRID_CELLS_X/Y/Z grid cells per axis
 *   MM_INFO_GRID_GLOBAL      rects every query tests (e.g. the maze floor)
 *   MM_INFO_GRID_BYTES       the grid image (cells, lists, records, leaf boxes)
 *   MM_INFO_GRID_INDEX_BYTES its cells + lists part
 *   MM_INFO_LEAN             1 if every rect has a compact record
 *   MM_INFO_DEPTH            BVH depth (max traversal stack entries)
 *   MM_INFO_DICT_OK          0 (dictionary-coded nodes were removed in round 6; the key is kept)
 *   MM_INFO_LAST_FORM        query method of the last wave-persistent launch (MM_OPT_TRAVERSAL value)
 *   MM_INFO_LAST_LDS_MODE    its LDS mode (trace_kernels.hip: 0, 1, 3 BVH; 11-14 grid)
 *   MM_INFO_GRID_FACES       1 if the grid cells carry per-face list ranges (64-bit cell words)
 *   MM_INFO_LAST_DEFER       1 if the last mm_trace_tile* call ran the mirror-tail rings
 *   MM_INFO_LAST_VGPRS       VGPRs per lane of the last wave-persistent kernel (code-object metadata)
 *   MM_INFO_LAST_SCRATCH     its private (scratch) bytes per lane: VGPR spills + traversal stack
 *   MM_INFO_LAST_STATIC_LDS  its static LDS bytes per block (the tail ring's words)
 *   MM_INFO_GRID_LDS_CAP     bytes the grid placements 11 / 14 stage into (their static LDS array without
 *                            tail rings; the grid builder's budget: no grid image is built larger)
 *   MM_INFO_GRID_FLAT        1 if the grid takes the maze forms (one y cell, compact 16-byte records + class table)
 *   MM_INFO_GRID_SLAB        1 if the two global rects are a floor / ceiling pair, sorted by y, a query tests one of
 *   MM_INFO_GRID_CLASSES     threshold classes of the compact records (0 without them)
 *   MM_INFO_LAST_KERNEL_FORM the internal form of the last wave-persistent launch: 5, 7, or the grid search's
 *                            11 plain, 12 slow, 13 wide, 14 wide + slow, 15..18 the same on a maze grid
 *                            (MM_INFO_LAST_FORM folds 11..18 to 11); -1 before the first such launch
 *   MM_INFO_LAST_RING        its tail-ring kind: 0 none, 1 records in global memory, 2 records in LDS */
#define MM_INFO_GRID_OK          1
#define MM_INFO_GRID_CELLS_X     2
#define MM_INFO_GRID_CELLS_Y     3
#define MM_INFO_GRID_CELLS_Z     4
#define MM_INFO_GRID_GLOBAL      5
#define MM_INFO_GRID_BYTES       6
#define MM_INFO_GRID_INDEX_BYTES 7
#define MM_INFO_LEAN             8
#define MM_INFO_DEPTH            9
#define MM_INFO_DICT_OK          10
#define MM_INFO_LAST_FORM        11
#define MM_INFO_LAST_LDS_MODE    12
#define MM_INFO_GRID_FACES       13
#define MM_INFO_LAST_DEFER       14
#define MM_INFO_LAST_VGPRS       15
#define MM_INFO_LAST_SCRATCH     16
#define MM_INFO_LAST_STATIC_LDS  17
#define MM_INFO_GRID_LDS_CAP     18
#define MM_INFO_GRID_FLAT        19
#define MM_INFO_GRID_SLAB        20
#define MM_INFO_GRID_CLASSES     21
#define MM_INFO_LAST_KERNEL_FORM 22
#define MM_INFO_LAST_RING        23
int  mm_scene_info(const mm_ctx* ctx, int key, double* value);

/* Host only, no context: 1 if the build holds the wave-persistent trace kernel for this LDS mode
 * (MM_INFO_LAST_LDS_MODE), internal form (MM_INFO_LAST_KERNEL_FORM) and tail-ring kind (MM_INFO_LAST_RING;
 * kinds 1 and 2 exist where the pair has a tail-deferral variant), else 0. */
int  mm_variant_built(int lds_mode, int form, int ring);

/* Diagnostics: record, for every wave of the wave-persistent kernel, four u64
 * into the device buffer `dev_buf` (n_waves x 4): entry time, LDS staging
 * done, exit time (wall_clock64 ticks, 100 MHz) and the number of 64-path
 * chunks it traced.  NULL turns it off (default).  scripts/timeline_probe.py */
int  mm_set_wave_timeline(mm_ctx* ctx, unsigned long long* dev_buf, uint32_t n_waves);

/* Wait for all work queued by this context; returns the error of the oldest
 * mm_trace_tile* call that failed on the GPU and was not reported yet. */
int  mm_sync(mm_ctx* ctx);

/* Asynchronous errors.  mm_trace_tile / mm_trace_tile_frames return before
 * the GPU runs them; each such call is numbered (1, 2, ...) and its launches
 * publish their error flags (traversal stack overflow, a tail-ring protocol
 * timeout, an injected fault) into host-mapped status words when they end.
 * A call that failed is reported -- its return code, and mm_last_error naming
 * "call #N (what it traced)" -- by the first of: the next mm_trace_tile* call
 * on the context (which is then not enqueued), mm_sync, or mm_call_status(N).
 * It is never attributed to a later call's own work.  (The reference has no
 * error path: a Metal command buffer fails silently, src/main.rs:893-894.) */
#define MM_PENDING 1
int  mm_last_call(const mm_ctx* ctx, uint64_t* call_id);
/* Without waiting: MM_OK (finished clean), MM_PENDING (still running) or the
 * call's error code (message in mm_last_error). */
int  mm_call_status(mm_ctx* ctx, uint64_t call_id);

/* Per-kernel timing of the dominant (ray-trace) kernel: when enabled, every
 * trace-kernel launch is bracketed by HIP events on the context's stream.
 * mm_kernel_timing syncs, returns the summed ms and the launch count since the
 * last reset, and optionally resets. */
int  mm_set_profiling(mm_ctx* ctx, int enable);
int  mm_kernel_timing(mm_ctx* ctx, float* total_ms, uint32_t* launches, int reset);

/* Device-side timing of the last mm_trace_tile / mm_trace_chunks call,
 * measured with HIP events on the context's stream (ms), and the number of
 * kernel launches it made. */
int  mm_last_timing(mm_ctx* ctx, float* ms, uint32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* MM_API_H */
