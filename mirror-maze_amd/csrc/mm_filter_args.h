// mm_filter_args.h — the argument checks of the frame filters' calls (mm_filters.hip: mm_denoise_frames,
// mm_accumulate_frames, mm_blend_pixels and their _var forms, mm_upsample_frames and mm_fill_pixels) as pure
// functions of the arguments: no context, no device, nothing dereferenced but the parameter structs.  Plain C++
// (no HIP), as mm_plan.h: stand-alone host programs test them (tests/filter_args, tests/upsample_args).
//
// One function per pair (the last two calls have one each).  `var` says which call of the pair it is and `name`
// is that call's name, the prefix of every message; what the variance call adds stands in branches of the one
// function.  A plain call's parameter and history structs come in the variance call's form (the members it
// lacks unread).  The checks run in the order include/mm_api.h lists them, and the first that fails gives the
// result.
#pragma once

#include <cstdint>
#include <string>

#include "mm_api.h"

namespace mm {

// Whether [a, a + na) and [b, b + nb) share a byte.
bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb);

// One device buffer of a call, as the alignment and overlap rules see it.  A null pointer -- a buffer the call
// may leave out -- is aligned and overlaps nothing.
struct FilterBuf {
    const void* ptr;
    uint64_t bytes;
    uint32_t align;
    bool output;
};
bool any_misaligned(const FilterBuf* bufs, size_t n);
// Whether an output of the table shares a byte with an input / with another output.
bool output_hits_input(const FilterBuf* bufs, size_t n);
bool outputs_overlap(const FilterBuf* bufs, size_t n);

struct ArgCheck {
    int code = MM_OK;  // else `error` is the text
    std::string error;
};

ArgCheck check_denoise(bool var, const char* name, const float* color, const mm_aov* guides, const float* vmean,
                       const mm_denoise_var_params* p, uint32_t n_frames, uint32_t w, uint32_t h, const void* out,
                       const float* var_out);

ArgCheck check_accumulate(bool var, const char* name, const mm_uniform* u, const mm_camera* cams, const float* color,
                          const mm_aov* guides, const float* vmean, const float* weight,
                          const mm_temporal_prev_var* prev, const mm_temporal_params* p, uint32_t n_frames, uint32_t x0,
                          uint32_t y0, uint32_t w, uint32_t h, const void* out, const float* var_out);

// MM_OK with n_pixels == 0 is the call that has nothing to do: the checks of the list's buffers are then not made.
ArgCheck check_blend(bool var, const char* name, const float* image, const float* var_image, uint32_t w, uint32_t h,
                     const uint32_t* pixels, const float* extra, const float* extra_vmean, uint64_t n_pixels, float m);

// The blocks of an mm_upsample_frames call (64 x 4 pixels each, every frame's in its one launch) and how many a
// launch holds: each is 64 threads wide, and a grid's threads along x stay below 2^32.
constexpr uint64_t kUpsampleMaxBlocks = (1ull << 26) - 1;
constexpr uint64_t upsample_blocks(uint32_t w, uint32_t h, uint32_t n_frames) {
    return (((uint64_t)w + 63) / 64) * (((uint64_t)h + 3) / 4) * n_frames;
}

ArgCheck check_upsample(const char* name, const float* low, const mm_aov* guides, const float* low_vmean,
                        const mm_upsample_params* p, uint32_t n_frames, uint32_t w, uint32_t h, const void* out,
                        const float* weight_out, const float* var_out);

// MM_OK with n_pixels == 0: as check_blend.
ArgCheck check_fill(const char* name, const float* image, const float* var_image, const float* weight_image,
                    uint32_t w, uint32_t h, const uint32_t* pixels, const float* extra, const float* extra_vmean,
                    uint64_t n_pixels, float m);

}  // namespace mm
