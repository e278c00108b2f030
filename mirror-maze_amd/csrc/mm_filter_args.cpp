// mm_filter_args.cpp — see mm_filter_args.h.
#include "mm_filter_args.h"

#include <cmath>

namespace mm {

bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

bool any_misaligned(const FilterBuf* bufs, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (reinterpret_cast<uintptr_t>(bufs[i].ptr) % bufs[i].align) return true;
    return false;
}

namespace {

// Whether some pair of the table's buffers, an output and (inputs) an input or (else) a later output, overlaps.
bool pair_overlaps(const FilterBuf* bufs, size_t n, bool inputs) {
    for (size_t i = 0; i < n; ++i)
        for (size_t j = inputs ? 0 : i + 1; j < n; ++j) {
            const FilterBuf &o = bufs[i], &b = bufs[j];
            if (!o.output || b.output == inputs || !o.ptr || !b.ptr) continue;
            if (ranges_overlap(o.ptr, o.bytes, b.ptr, b.bytes)) return true;
        }
    return false;
}

ArgCheck bad(const char* name, const char* what) { return {MM_ERR_INVALID, std::string(name) + ": " + what}; }

// The frame shape both frame calls take: n_frames frames of w x h pixels.
bool too_many_pixels(uint64_t n_pix, uint32_t n_frames) {
    return n_pix > 0x7FFFFFFFull || n_pix * n_frames > (1ull << 40);
}

}  // namespace

bool output_hits_input(const FilterBuf* bufs, size_t n) { return pair_overlaps(bufs, n, true); }
bool outputs_overlap(const FilterBuf* bufs, size_t n) { return pair_overlaps(bufs, n, false); }

ArgCheck check_denoise(bool var, const char* name, const float* color, const mm_aov* guides, const float* vmean,
                       const mm_denoise_var_params* p, uint32_t n_frames, uint32_t w, uint32_t h, const void* out,
                       const float* var_out) {
    if (!p || !guides || !color || (var && !vmean) || !out) return bad(name, "null argument");
    if (!guides->normal_depth || !guides->albedo || !guides->id)
        return bad(name, "all three guide buffers are required");
    if (p->n_passes < 1 || p->n_passes > MM_DENOISE_MAX_PASSES) return bad(name, "n_passes must be 1..8");
    if (p->flags & ~MM_DN_RGBA8) return bad(name, "unknown flags");
    if (var) {
        if (p->reserved != 0) return bad(name, "reserved must be 0");
        if (p->sigma_l > 0.0f && (!(p->eps_l > 0.0f) || !std::isfinite(p->eps_l)))
            return bad(name, "eps_l must be positive and finite when sigma_l > 0");
    }
    if (w == 0 || h == 0 || n_frames == 0) return bad(name, "empty tile or no frames");
    const bool rgba8 = (p->flags & MM_DN_RGBA8) != 0;
    // (the byte counts mean something once too_many_pixels has passed; until then only the alignments are read)
    const uint64_t n_pix = (uint64_t)w * h, n_all = n_pix * n_frames;
    const FilterBuf bufs[] = {{color, n_all * 16, 16, false},
                              {guides->normal_depth, n_all * 16, 16, false},
                              {guides->albedo, n_all * 16, 16, false},
                              {guides->id, n_all * 4, 4, false},
                              {out, n_all * (rgba8 ? 4 : 16), rgba8 ? 4u : 16u, true},
                              // the variance call's
                              {vmean, n_all * 4, 4, false},
                              {var_out, n_all * 4, 4, true}};
    const size_t n_bufs = var ? 7 : 5;
    if (any_misaligned(bufs, n_bufs))
        return bad(name, var ? "misaligned buffer (float4: 16 bytes; id, variance and RGBA8: 4)"
                             : "misaligned buffer (float4: 16 bytes, id and RGBA8: 4)");
    if (too_many_pixels(n_pix, n_frames)) return bad(name, "more pixels than one call holds");
    if (output_hits_input(bufs, n_bufs))
        return bad(name, var ? "an output overlaps an input" : "the output overlaps an input");
    if (outputs_overlap(bufs, n_bufs)) return bad(name, "the two outputs overlap");
    return {};
}

ArgCheck check_accumulate(bool var, const char* name, const mm_uniform* u, const mm_camera* cams, const float* color,
                          const mm_aov* guides, const float* vmean, const float* weight,
                          const mm_temporal_prev_var* prev, const mm_temporal_params* p, uint32_t n_frames, uint32_t x0,
                          uint32_t y0, uint32_t w, uint32_t h, const void* out, const float* var_out) {
    if (!u || !cams || !color || !guides || !p || !out || (var && (!vmean || !var_out)))
        return bad(name, "null argument");
    if (!guides->normal_depth || !guides->albedo || !guides->id)
        return bad(name, "all three guide buffers are required");
    if (prev && (!prev->color || !prev->guides.normal_depth || !prev->guides.albedo || !prev->guides.id ||
                 (var && !prev->var)))
        return bad(name, var ? "prev needs its colour, all three guide buffers and its variance"
                             : "prev needs its colour and all three guide buffers");
    if (p->n_max < 1 || p->n_max > 65535) return bad(name, "n_max must be 1..65535");
    if (!(p->tol_z > 0.0f) || !std::isfinite(p->tol_z)) return bad(name, "tol_z must be positive and finite");
    if (!(p->w_min > 0.0f && p->w_min <= 1.0f)) return bad(name, "w_min must be in (0, 1]");
    if (p->flags) return bad(name, "unknown flags");
    if (w == 0 || h == 0 || n_frames == 0) return bad(name, "empty tile or no frames");
    // (the byte counts: as in check_denoise.  The history frame's buffers are one frame each.)
    const uint64_t n_pix = (uint64_t)w * h, n_all = n_pix * n_frames;
    const mm_temporal_prev_var none{};
    const mm_temporal_prev_var& h0 = prev ? *prev : none;
    const FilterBuf bufs[] = {{color, n_all * 16, 16, false},
                              {guides->normal_depth, n_all * 16, 16, false},
                              {guides->albedo, n_all * 16, 16, false},
                              {guides->id, n_all * 4, 4, false},
                              {h0.color, n_pix * 16, 16, false},
                              {h0.guides.normal_depth, n_pix * 16, 16, false},
                              {h0.guides.albedo, n_pix * 16, 16, false},
                              {h0.guides.id, n_pix * 4, 4, false},
                              {out, n_all * 16, 16, true},
                              // the variance call's
                              {vmean, n_all * 4, 4, false},
                              {weight, n_all * 4, 4, false},
                              {h0.var, n_pix * 4, 4, false},
                              {var_out, n_all * 4, 4, true}};
    const size_t n_bufs = var ? 13 : 9;
    if (any_misaligned(bufs, n_bufs))
        return bad(name, var ? "misaligned buffer (float4: 16 bytes, id and variances: 4)"
                             : "misaligned buffer (float4: 16 bytes, id: 4)");
    if (too_many_pixels(n_pix, n_frames)) return bad(name, "more pixels than one call holds");
    if ((uint64_t)x0 + w > (1ull << 24) || (uint64_t)y0 + h > (1ull << 24))
        return bad(name, "the window ends beyond pixel 2^24");
    if (output_hits_input(bufs, n_bufs))
        return bad(name, var ? "an output overlaps an input" : "the output overlaps an input");
    if (outputs_overlap(bufs, n_bufs)) return bad(name, "the two outputs overlap");
    return {};
}

ArgCheck check_blend(bool var, const char* name, const float* image, const float* var_image, uint32_t w, uint32_t h,
                     const uint32_t* pixels, const float* extra, const float* extra_vmean, uint64_t n_pixels, float m) {
    if (!image || (var && !var_image)) return bad(name, var ? "null image or variance" : "null image");
    const uint64_t n_pix = (uint64_t)w * h;
    if (w == 0 || h == 0 || n_pix > 0x7FFFFFFFull) return bad(name, "empty window or more than 2^31 - 1 pixels");
    if (!(m > 0.0f) || !std::isfinite(m)) return bad(name, "m must be positive and finite");
    // the window's images are read and written in place: outputs, which no input may touch
    const FilterBuf window[] = {{image, n_pix * 16, 16, true}, {var ? var_image : nullptr, n_pix * 4, 4, true}};
    if (any_misaligned(window, 2)) return bad(name, var ? "misaligned image or variance" : "misaligned image");
    if (outputs_overlap(window, 2)) return bad(name, "var_dev overlaps the image");
    if (n_pixels == 0) return {};
    if (!pixels || !extra || (var && !extra_vmean)) return bad(name, "null argument");
    // one image of the window, then the list's buffers (their byte counts: once n_pixels has passed its bound)
    FilterBuf t[] = {window[0],
                     {extra, n_pixels * 16, 16, false},
                     {pixels, n_pixels * 8, 8, false},
                     {var ? extra_vmean : nullptr, n_pixels * 4, 4, false}};
    if (any_misaligned(t + 1, var ? 3 : 2))
        return bad(name, var ? "misaligned buffer (float4: 16 bytes, the list: 8, variances: 4)"
                             : "misaligned buffer (float4: 16 bytes, the list: 8)");
    if (n_pixels > (1ull << 38)) return bad(name, "more entries than one launch holds");
    // (mm_blend_pixels tests extra_dev alone against the image)
    if (!var) return output_hits_input(t, 2) ? bad(name, "extra_dev overlaps the image") : ArgCheck{};
    if (output_hits_input(t, 4)) return bad(name, "an input overlaps the image");
    t[0] = window[1];
    if (output_hits_input(t, 4)) return bad(name, "an input overlaps var_dev");
    return {};
}

ArgCheck check_upsample(const char* name, const float* low, const mm_aov* guides, const float* low_vmean,
                        const mm_upsample_params* p, uint32_t n_frames, uint32_t w, uint32_t h, const void* out,
                        const float* weight_out, const float* var_out) {
    if (!p || !guides || !low || !out) return bad(name, "null argument");
    if (!guides->normal_depth || !guides->albedo || !guides->id)
        return bad(name, "all three guide buffers are required");
    if (p->scale != 2 && p->scale != 4 && p->scale != 8) return bad(name, "scale must be 2, 4 or 8");
    if (!(p->w_min > 0.0f && p->w_min <= 1.0f)) return bad(name, "w_min must be in (0, 1]");
    if (p->flags) return bad(name, "unknown flags");
    if (p->reserved != 0) return bad(name, "reserved must be 0");
    if (w == 0 || h == 0 || n_frames == 0) return bad(name, "empty tile or no frames");
    // (the byte counts: as in check_denoise.  The lattice's buffers hold ceil(w / scale) x ceil(h / scale) pixels.)
    const uint64_t n_pix = (uint64_t)w * h, n_all = n_pix * n_frames;
    const uint64_t n_low = (((uint64_t)w + p->scale - 1) / p->scale) * (((uint64_t)h + p->scale - 1) / p->scale) * n_frames;
    const FilterBuf bufs[] = {{low, n_low * 16, 16, false},
                              {guides->normal_depth, n_all * 16, 16, false},
                              {guides->albedo, n_all * 16, 16, false},
                              {guides->id, n_all * 4, 4, false},
                              {low_vmean, n_low * 4, 4, false},
                              {out, n_all * 16, 16, true},
                              {weight_out, n_all * 4, 4, true},
                              {var_out, n_all * 4, 4, true}};
    const size_t n_bufs = sizeof bufs / sizeof bufs[0];
    if (any_misaligned(bufs, n_bufs))
        return bad(name, "misaligned buffer (float4: 16 bytes; id, variances and weights: 4)");
    if (var_out && !low_vmean) return bad(name, "var_out_dev needs low_vmean_dev");
    if (too_many_pixels(n_pix, n_frames)) return bad(name, "more pixels than one call holds");
    if (upsample_blocks(w, h, n_frames) > kUpsampleMaxBlocks) return bad(name, "more blocks than one launch holds");
    if (output_hits_input(bufs, n_bufs)) return bad(name, "an output overlaps an input");
    if (outputs_overlap(bufs, n_bufs)) return bad(name, "two outputs overlap");
    return {};
}

ArgCheck check_fill(const char* name, const float* image, const float* var_image, const float* weight_image,
                    uint32_t w, uint32_t h, const uint32_t* pixels, const float* extra, const float* extra_vmean,
                    uint64_t n_pixels, float m) {
    if (!image) return bad(name, "null image");
    const uint64_t n_pix = (uint64_t)w * h;
    if (w == 0 || h == 0 || n_pix > 0x7FFFFFFFull) return bad(name, "empty window or more than 2^31 - 1 pixels");
    if (!(m > 0.0f) || !std::isfinite(m)) return bad(name, "m must be positive and finite");
    // the window's images are written in place: outputs, which no input may touch
    const FilterBuf window[] = {{image, n_pix * 16, 16, true},
                                {var_image, n_pix * 4, 4, true},
                                {weight_image, n_pix * 4, 4, true}};
    if (any_misaligned(window, 3)) return bad(name, "misaligned image, variance or weight");
    if (outputs_overlap(window, 3)) return bad(name, "two of image_dev, var_dev and weight_dev overlap");
    if (n_pixels == 0) return {};
    if (!pixels || !extra) return bad(name, "null argument");
    if ((var_image != nullptr) != (extra_vmean != nullptr))
        return bad(name, "var_dev and extra_vmean_dev go together");
    // one image of the window, then the list's buffers (their byte counts: once n_pixels has passed its bound)
    FilterBuf t[] = {window[0],
                     {extra, n_pixels * 16, 16, false},
                     {pixels, n_pixels * 8, 8, false},
                     {extra_vmean, n_pixels * 4, 4, false}};
    if (any_misaligned(t + 1, 3)) return bad(name, "misaligned buffer (float4: 16 bytes, the list: 8, variances: 4)");
    if (n_pixels > (1ull << 38)) return bad(name, "more entries than one launch holds");
    if (output_hits_input(t, 4)) return bad(name, "an input overlaps the image");
    t[0] = window[1];
    if (output_hits_input(t, 4)) return bad(name, "an input overlaps var_dev");
    t[0] = window[2];
    if (output_hits_input(t, 4)) return bad(name, "an input overlaps weight_dev");
    return {};
}

}  // namespace mm
