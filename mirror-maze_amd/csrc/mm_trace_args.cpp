// mm_trace_args.cpp — see mm_trace_args.h.
#include "mm_trace_args.h"

#include <algorithm>
#include <string>

#include "mm_plan.h"

namespace mm {

namespace {

ArgCheck bad(const char* name, const std::string& what) { return {MM_ERR_INVALID, std::string(name) + ": " + what}; }

bool misaligned(const void* p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

}  // namespace

ArgCheck check_tile(const char* name, const mm_uniform* u, const mm_ext* e, uint32_t mirror_limit, uint32_t x0,
                    uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride) {
    if (!(u->view_w >= 1.0f && u->view_w <= 65536.0f && u->view_h >= 1.0f && u->view_h <= 65536.0f))
        return bad(name, "bad view size");
    const uint32_t W = (uint32_t)u->view_w, H = (uint32_t)u->view_h;
    if (w == 0 || h == 0 || y_stride == 0 || (e && (e->spp == 0 || e->spp > 4096)))
        return bad(name, e ? "empty tile or bad spp" : "empty tile");
    // the tail records pack bounces | mirror hits << 16 (trace_kernels.hip tail_store)
    if ((e && e->bounce_limit > 32767) || mirror_limit > 32767)
        return bad(name, e ? "bounce or mirror limit above 32767" : "mirror limit above 32767");
    if ((uint64_t)x0 + w > W || (uint64_t)y0 + (uint64_t)(h - 1) * y_stride >= H)
        return bad(name, "tile outside the frame");
    return {};
}

ArgCheck check_var(const char* name, const mm_ext* e, const void* out_dev, uint64_t out_bytes, const float* var_dev,
                   uint64_t n) {
    if (e->spp < 2) return bad(name, "a sample variance needs spp >= 2");
    if (e->flags & MM_EXT_ACCUMULATE) return bad(name, "MM_EXT_ACCUMULATE is not supported");
    if (!var_dev) return bad(name, "null var_dev");
    if (misaligned(var_dev, 4)) return bad(name, "var_dev not 4-byte aligned");
    if (ranges_overlap(out_dev, out_bytes, var_dev, n * 4)) return bad(name, "var_dev overlaps out_dev");
    return {};
}

ArgCheck check_trace_tile(const char* multi_fn, bool var, const mm_uniform* u, const mm_ext* e, uint32_t n_frames,
                          uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, const void* out_dev,
                          const float* var_dev) {
    const char* name = "mm_trace_tile";
    if (!u || !e || !out_dev) return bad(name, "null argument");
    ArgCheck ck = check_tile(name, u, e, e->mirror_limit, x0, y0, w, h, y_stride);
    if (ck.code != MM_OK) return ck;
    if (n_frames == 0) return bad(multi_fn, "no frames");
    // MM_EXT_RGBA8: 4-byte RGBA8 pixels (the fused texture-write conversion) instead of float4
    const bool rgba8 = (e->flags & MM_EXT_RGBA8) != 0;
    if (rgba8 && (e->flags & MM_EXT_ACCUMULATE)) return bad(name, "MM_EXT_RGBA8 frames cannot accumulate");
    const size_t out_bpp = rgba8 ? 4 : 16;
    // the stores are out_bpp wide (a float4 per pixel, or one RGBA8 word): the output must be aligned to that
    if (misaligned(out_dev, out_bpp)) return bad(name, "output not " + std::to_string(out_bpp) + "-byte aligned");
    if (var) {
        // (elements in all, capped where the plan refuses the launch anyway: the byte counts fit 64 bits)
        const uint64_t n_all = std::min<uint64_t>((uint64_t)w * h, (1ull << 40) / n_frames) * n_frames;
        return check_var("mm_trace_tile_var", e, out_dev, n_all * out_bpp, var_dev, n_all);
    }
    return {};
}

ArgCheck check_trace_lists(bool lists, bool var, const mm_uniform* u, const mm_ext* e, const uint64_t* offsets,
                           uint32_t n_lists, const uint32_t* pixels_dev, const void* out_dev, const float* var_dev,
                           uint64_t& n_entries) {
    const char* name = lists ? "mm_trace_pixel_lists" : "mm_trace_pixels";
    n_entries = lists ? 0 : offsets[1];
    std::string why;
    if (lists)
        if (int rc = lists_total(offsets, n_lists, n_entries, why)) return {rc, why};
    if (n_entries == 0) return {};
    if (!u || !e || !pixels_dev || !out_dev) return bad(name, "null argument");
    // (the view, spp and the limits: the tile calls' checks, on a one-pixel tile)
    ArgCheck ck = check_tile(name, u, e, e->mirror_limit, 0, 0, 1, 1, 1);
    if (ck.code != MM_OK) return ck;
    const bool rgba8 = (e->flags & MM_EXT_RGBA8) != 0;
    if (rgba8 && (e->flags & MM_EXT_ACCUMULATE)) return bad(name, "MM_EXT_RGBA8 results cannot accumulate");
    const size_t out_bpp = rgba8 ? 4 : 16;
    if (misaligned(pixels_dev, 8) || misaligned(out_dev, out_bpp))
        return bad(name, std::string(lists ? "lists" : "list") + " not 8-byte or output not " +
                             std::to_string(out_bpp) + "-byte aligned");
    if (var) {
        if (n_entries > 0xFFFFFFFFull)  // (the plan's own refusal, ahead of the byte counts below)
            return bad(name, "more paths than one launch holds (2^32)");
        return check_var(lists ? name : "mm_trace_pixels_var", e, out_dev, n_entries * out_bpp, var_dev, n_entries);
    }
    return {};
}

ArgCheck check_trace_rays(const mm_ext* e, uint32_t ray_flags, const float* rays_dev, uint64_t n_rays,
                          const void* out_dev, const float* var_dev) {
    const char* name = "mm_trace_rays";
    if (n_rays == 0) return {};
    if (!e || !rays_dev || !out_dev) return bad(name, "null argument");
    const bool rgba8 = (e->flags & MM_EXT_RGBA8) != 0;
    const size_t out_bpp = rgba8 ? 4 : 16;
    if (misaligned(rays_dev, 16) || misaligned(out_dev, out_bpp))
        return bad(name, "rays not 16-byte or output not " + std::to_string(out_bpp) + "-byte aligned");
    if (ray_flags & ~MM_RAYS_JITTER) return bad(name, "unknown ray_flags");
    if (e->spp == 0 || e->spp > 4096) return bad(name, "bad spp");
    if (e->bounce_limit > 32767 || e->mirror_limit > 32767) return bad(name, "bounce or mirror limit above 32767");
    if (rgba8 && (e->flags & MM_EXT_ACCUMULATE)) return bad(name, "MM_EXT_RGBA8 results cannot accumulate");
    if (var_dev) {
        if (n_rays > 0xFFFFFFFFull)  // (the plan's own refusal, ahead of the byte counts below)
            return bad(name, "more paths than one launch holds (2^32)");
        return check_var(name, e, out_dev, n_rays * out_bpp, var_dev, n_rays);
    }
    return {};
}

ArgCheck check_trace_aov(const mm_uniform* u, bool has_cams, uint32_t n_frames, uint32_t mirror_limit, uint32_t x0,
                         uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, const mm_aov* out) {
    const char* name = "mm_trace_aov";
    if (!u || !out) return bad(name, "null argument");
    if (!out->normal_depth && !out->albedo && !out->id) return bad(name, "no output");
    if (n_frames == 0) return bad(name, "no frames");
    if (!has_cams && n_frames > 1) return bad(name, "several frames need their cameras");
    ArgCheck ck = check_tile(name, u, nullptr, mirror_limit, x0, y0, w, h, y_stride);
    if (ck.code != MM_OK) return ck;
    if (misaligned(out->normal_depth, 16) || misaligned(out->albedo, 16) || misaligned(out->id, 4))
        return bad(name, "float4 outputs not 16-byte or id not 4-byte aligned");
    const uint64_t n_pix = (uint64_t)w * h;
    if (n_pix > 0x7FFFFFFFull || (n_pix + 255) / 256 * n_frames > 0x7FFFFFFFull)
        return bad(name, "more pixels than one launch holds");
    return {};
}

ArgCheck check_query_rays(const float* rays_dev, uint64_t n_rays, const void* hits_dev, uint64_t max_rays) {
    const char* name = "mm_query_rays";
    if (n_rays == 0) return {};
    if (!rays_dev || !hits_dev) return bad(name, "null argument");
    if (misaligned(rays_dev, 16) || misaligned(hits_dev, 8))
        return bad(name, "rays not 16-byte or hits not 8-byte aligned");
    if (n_rays > max_rays) return bad(name, "more rays than one launch holds");
    return {};
}

}  // namespace mm
