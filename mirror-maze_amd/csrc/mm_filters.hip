// mm_filters.hip — the frame filters of the C ABI (include/mm_api.h): mm_denoise_frames, mm_accumulate_frames,
// mm_blend_pixels and their _var forms, mm_upsample_frames and mm_fill_pixels.  One implementation per pair: the
// variance call is the plain call with more buffers, and what it adds stands under `var`.  A plain call's
// parameter and history structs are widened to the variance call's at the entry point.
//
// Every call checks its arguments first (mm_filter_args.h), and none of the checks needs the context: a binding
// can be tested without a GPU, and a null context is refused only after them.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mm_api.h"
#include "mm_ctx.h"
#include "mm_filter_args.h"
#include "mm_launch.h"

using namespace mm;

namespace {

// What a denoise call needs before its passes: the intermediate images a frame's passes alternate between (one
// frame each; `var`: and the variance images beside them), the call's packed key records, filled here, and its
// place after the last call's kernels.  The scratch, its event and its stream bookkeeping are one for both
// calls: they take turns on it in the order they were made.
int dn_begin(mm_ctx* c, bool var, const mm_aov* guides, uint32_t n_passes, uint64_t n_pix, uint64_t n_all) {
    if (n_passes > 1) {
        const size_t sides = n_passes > 2 ? 2 : 1;
        if (int rc = ensure_idle(c, c->d_dn_img, c->dn_img_cap, sides * (size_t)n_pix)) return rc;
        if (var)
            if (int rc = ensure_idle(c, c->d_dn_var, c->dn_var_cap, sides * (size_t)n_pix)) return rc;
    }
    if (int rc = ensure_idle(c, c->d_dn_keys, c->dn_keys_cap, (size_t)n_all)) return rc;
    if (!c->dn_done) HIPC(c, hipEventCreateWithFlags(&c->dn_done, hipEventDisableTiming));
    if (c->dn_pending && c->dn_stream != c->stream) HIPC(c, hipStreamWaitEvent(c->stream, c->dn_done, 0));
    HIPC(c, launch_denoise_keys(reinterpret_cast<const float4*>(guides->albedo), guides->id, c->d_dn_keys,
                                (size_t)n_all, c->stream));
    c->dn_pending = true;
    c->dn_stream = c->stream;
    return MM_OK;
}

// Pass: DnPass (mm_denoise_frames) or DnVarPass (mm_denoise_frames_var), whose shared members are named alike.
template <typename Pass>
int denoise_impl(mm_ctx* c, const char* name, const float* color_dev, const mm_aov* guides, const float* vmean_dev,
                 const mm_denoise_var_params* p, uint32_t n_frames, uint32_t w, uint32_t h, void* out_dev,
                 float* var_out_dev) {
    constexpr bool var = std::is_same_v<Pass, DnVarPass>;
    const ArgCheck ck = check_denoise(var, name, color_dev, guides, vmean_dev, p, n_frames, w, h, out_dev, var_out_dev);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (!c) return MM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    const bool rgba8 = (p->flags & MM_DN_RGBA8) != 0;
    const uint32_t n_passes = p->n_passes;
    const uint64_t n_pix = (uint64_t)w * h;
    if (int rc = dn_begin(c, var, guides, n_passes, n_pix, n_pix * n_frames)) return rc;
    // All passes of a frame run before the next frame's: the two intermediate images are one frame each (a
    // launch per pass over all frames measured 1.4 % slower and needs 2 x n_frames images).
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * n_pix;
        Pass a;
        a.nd = reinterpret_cast<const float4*>(guides->normal_depth) + o;
        a.keys = c->d_dn_keys + o;
        a.w = w; a.h = h;
        a.sigma_z = p->sigma_z; a.sigma_l = p->sigma_l;
        a.in = reinterpret_cast<const float4*>(color_dev) + o;
        if constexpr (var) {
            a.eps_l = p->eps_l;
            a.vin = vmean_dev + o;
        }
        for (uint32_t i = 0; i < n_passes; ++i) {
            const bool last = i + 1 == n_passes;
            const size_t side = (size_t)(i & 1u) * n_pix;
            a.s = 1u << i;
            a.rgba8 = last && rgba8;
            if (last) a.out = rgba8 ? (void*)(reinterpret_cast<uint8_t*>(out_dev) + o * 4)
                                    : (void*)(reinterpret_cast<float4*>(out_dev) + o);
            else a.out = c->d_dn_img + side;
            if constexpr (var) {
                a.vout = last ? (var_out_dev ? var_out_dev + o : nullptr) : c->d_dn_var + side;
                HIPC(c, launch_denoise_var_pass(a, c->stream));
                a.vin = a.vout;
            } else {
                a.sl = p->sigma_l * (1.0f / (float)a.s);
                HIPC(c, launch_denoise_pass(a, c->stream));
            }
            a.in = reinterpret_cast<const float4*>(a.out);
        }
    }
    HIPC(c, hipEventRecord(c->dn_done, c->stream));
    return MM_OK;
}

int accumulate_impl(mm_ctx* c, bool var, const char* name, const mm_uniform* u, const mm_camera* cams,
                    const float* color_dev, const mm_aov* guides, const float* vmean_dev, const float* weight_dev,
                    const mm_temporal_prev_var* prev, const mm_temporal_params* p, uint32_t n_frames, uint32_t x0,
                    uint32_t y0, uint32_t w, uint32_t h, void* out_dev, float* var_out_dev) {
    const ArgCheck ck = check_accumulate(var, name, u, cams, color_dev, guides, vmean_dev, weight_dev, prev, p, n_frames,
                                         x0, y0, w, h, out_dev, var_out_dev);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (!c) return MM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    // One launch per frame, in stream order: frame f reads frame f - 1's output (`var`: its colour and its
    // variance), which the kernel boundary makes visible.  The cameras travel in the launches' arguments, so
    // `cams` is consumed when this returns and the call keeps no scratch.
    const uint64_t n_pix = (uint64_t)w * h;
    TpFrameVar b;
    TpFrame& a = b.f;
    a.view_w = u->view_w; a.view_h = u->view_h;
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h;
    a.n_max = (float)p->n_max; a.tol_z = p->tol_z; a.w_min = p->w_min;
    if (prev) {
        a.h_color = reinterpret_cast<const float4*>(prev->color);
        a.h_nd = reinterpret_cast<const float4*>(prev->guides.normal_depth);
        a.h_al = reinterpret_cast<const float4*>(prev->guides.albedo);
        a.h_id = prev->guides.id;
        a.h_cam = prev->cam;
        b.h_var = prev->var;
    }
    for (uint32_t f = 0; f < n_frames; ++f) {
        const size_t o = (size_t)f * n_pix;
        a.color = reinterpret_cast<const float4*>(color_dev) + o;
        a.nd = reinterpret_cast<const float4*>(guides->normal_depth) + o;
        a.al = reinterpret_cast<const float4*>(guides->albedo) + o;
        a.id = guides->id + o;
        a.out = reinterpret_cast<float4*>(out_dev) + o;
        a.cam = cams[f];
        if (var) {
            b.vmean = vmean_dev + o;
            b.weight = weight_dev ? weight_dev + o : nullptr;
            b.vout = var_out_dev + o;
            HIPC(c, launch_temporal_frame_var(b, c->stream));
        } else {
            HIPC(c, launch_temporal_frame(a, c->stream));
        }
        a.h_color = a.out; a.h_nd = a.nd; a.h_al = a.al; a.h_id = a.id;
        a.h_cam = a.cam;
        b.h_var = b.vout;
    }
    return MM_OK;
}

int blend_impl(mm_ctx* c, bool var, const char* name, float* image_dev, float* var_dev, uint32_t x0, uint32_t y0,
               uint32_t w, uint32_t h, const uint32_t* pixels_dev, const float* extra_dev, const float* extra_vmean_dev,
               uint64_t n_pixels, float m) {
    const ArgCheck ck = check_blend(var, name, image_dev, var_dev, w, h, pixels_dev, extra_dev, extra_vmean_dev,
                                    n_pixels, m);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (!c) return MM_ERR_INVALID;
    if (n_pixels == 0) return MM_OK;
    HIPC(c, hipSetDevice(c->device));
    TpBlendVar v;
    TpBlend& b = v.b;
    b.image = reinterpret_cast<float4*>(image_dev);
    b.pixels = reinterpret_cast<const uint2*>(pixels_dev);
    b.extra = reinterpret_cast<const float4*>(extra_dev);
    b.n = n_pixels;
    b.x0 = x0; b.y0 = y0; b.w = w; b.h = h;
    b.m = m;
    v.var = var_dev;
    v.extra_vmean = extra_vmean_dev;
    if (var) HIPC(c, launch_blend_pixels_var(v, c->stream));
    else HIPC(c, launch_blend_pixels(b, c->stream));
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_denoise_frames(mm_ctx* c, const float* color_dev, const mm_aov* guides, const mm_denoise_params* p,
                      uint32_t n_frames, uint32_t w, uint32_t h, void* out_dev) {
    const mm_denoise_var_params pv = p ? mm_denoise_var_params{p->n_passes, p->sigma_z, p->sigma_l, 0.0f, p->flags, 0}
                                       : mm_denoise_var_params{};
    return denoise_impl<DnPass>(c, "mm_denoise_frames", color_dev, guides, nullptr, p ? &pv : nullptr, n_frames, w, h,
                                out_dev, nullptr);
}

int mm_denoise_frames_var(mm_ctx* c, const float* color_dev, const mm_aov* guides, const float* vmean_dev,
                          const mm_denoise_var_params* p, uint32_t n_frames, uint32_t w, uint32_t h, void* out_dev,
                          float* var_out_dev) {
    return denoise_impl<DnVarPass>(c, "mm_denoise_frames_var", color_dev, guides, vmean_dev, p, n_frames, w, h, out_dev,
                                   var_out_dev);
}

int mm_accumulate_frames(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const float* color_dev,
                         const mm_aov* guides, const mm_temporal_prev* prev, const mm_temporal_params* p,
                         uint32_t n_frames, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* out_dev) {
    const mm_temporal_prev_var pv = prev ? mm_temporal_prev_var{prev->color, prev->guides, prev->cam, nullptr}
                                         : mm_temporal_prev_var{};
    return accumulate_impl(c, false, "mm_accumulate_frames", u, cams, color_dev, guides, nullptr, nullptr,
                           prev ? &pv : nullptr, p, n_frames, x0, y0, w, h, out_dev, nullptr);
}

int mm_accumulate_frames_var(mm_ctx* c, const mm_uniform* u, const mm_camera* cams, const float* color_dev,
                             const mm_aov* guides, const float* vmean_dev, const float* weight_dev,
                             const mm_temporal_prev_var* prev, const mm_temporal_params* p, uint32_t n_frames,
                             uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* out_dev, float* var_out_dev) {
    return accumulate_impl(c, true, "mm_accumulate_frames_var", u, cams, color_dev, guides, vmean_dev, weight_dev, prev,
                           p, n_frames, x0, y0, w, h, out_dev, var_out_dev);
}

int mm_blend_pixels(mm_ctx* c, float* image_dev, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                    const uint32_t* pixels_dev, const float* extra_dev, uint64_t n_pixels, float m) {
    return blend_impl(c, false, "mm_blend_pixels", image_dev, nullptr, x0, y0, w, h, pixels_dev, extra_dev, nullptr,
                      n_pixels, m);
}

int mm_blend_pixels_var(mm_ctx* c, float* image_dev, float* var_dev, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                        const uint32_t* pixels_dev, const float* extra_dev, const float* extra_vmean_dev,
                        uint64_t n_pixels, float m) {
    return blend_impl(c, true, "mm_blend_pixels_var", image_dev, var_dev, x0, y0, w, h, pixels_dev, extra_dev,
                      extra_vmean_dev, n_pixels, m);
}

int mm_upsample_frames(mm_ctx* c, const float* low_dev, const mm_aov* guides, const float* low_vmean_dev,
                       const mm_upsample_params* p, uint32_t n_frames, uint32_t w, uint32_t h, void* out_dev,
                       float* weight_out_dev, float* var_out_dev) {
    const ArgCheck ck = check_upsample("mm_upsample_frames", low_dev, guides, low_vmean_dev, p, n_frames, w, h, out_dev,
                                       weight_out_dev, var_out_dev);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (!c) return MM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    UpFrames a;
    a.low = reinterpret_cast<const float4*>(low_dev);
    a.vlow = low_vmean_dev;
    a.nd = reinterpret_cast<const float4*>(guides->normal_depth);
    a.al = reinterpret_cast<const float4*>(guides->albedo);
    a.id = guides->id;
    a.out = reinterpret_cast<float4*>(out_dev);
    a.wout = weight_out_dev;
    a.vout = var_out_dev;
    a.w = w; a.h = h;
    a.lw = (w + p->scale - 1) / p->scale; a.lh = (h + p->scale - 1) / p->scale;  // (w, h < 2^31: no overflow)
    a.n_frames = n_frames;
    a.shift = p->scale == 2 ? 1u : p->scale == 4 ? 2u : 3u;
    a.inv_s = 1.0f / (float)p->scale;
    a.w_min = p->w_min;
    a.lds = c->opt_upsample_lds;
    HIPC(c, launch_upsample_frames(a, c->stream));
    return MM_OK;
}

int mm_fill_pixels(mm_ctx* c, float* image_dev, float* var_dev, float* weight_dev, uint32_t x0, uint32_t y0, uint32_t w,
                   uint32_t h, const uint32_t* pixels_dev, const float* extra_dev, const float* extra_vmean_dev,
                   uint64_t n_pixels, float m) {
    const ArgCheck ck = check_fill("mm_fill_pixels", image_dev, var_dev, weight_dev, w, h, pixels_dev, extra_dev,
                                   extra_vmean_dev, n_pixels, m);
    if (ck.code != MM_OK) return fail(c, ck.code, ck.error);
    if (!c) return MM_ERR_INVALID;
    if (n_pixels == 0) return MM_OK;
    HIPC(c, hipSetDevice(c->device));
    UpFill b;
    b.image = reinterpret_cast<float4*>(image_dev);
    b.var = var_dev;
    b.weight = weight_dev;
    b.pixels = reinterpret_cast<const uint2*>(pixels_dev);
    b.extra = reinterpret_cast<const float4*>(extra_dev);
    b.extra_vmean = extra_vmean_dev;
    b.n = n_pixels;
    b.x0 = x0; b.y0 = y0; b.w = w; b.h = h;
    b.m = m;
    HIPC(c, launch_fill_pixels(b, c->stream));
    return MM_OK;
}

}  // extern "C"
