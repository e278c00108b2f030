// mm_trace_args.h — the argument checks of the trace and query calls (mm_trace_calls.hip) as pure functions of
// the arguments, in the manner of mm_filter_args.h (whose ArgCheck and ranges_overlap they use): no context, no
// device, nothing dereferenced but the parameter structs and a list call's offsets.  Plain C++ (no HIP): a
// stand-alone host program tests them (tests/trace_args).
//
// They cover what a call checks between "a scene is uploaded" and hipSetDevice; the null context, an earlier
// call's failure and the missing scene stay with the calls.  One function per family, the variance call a branch
// of it.  The first check that fails gives the result.
#pragma once

#include <cstdint>

#include "mm_api.h"
#include "mm_filter_args.h"

namespace mm {

// The view and tile checks shared by the trace calls; `name` prefixes the messages.  e: the sampling
// parameters of a call that has them (mm_trace_tile*), else null and the call's own mirror limit.
ArgCheck check_tile(const char* name, const mm_uniform* u, const mm_ext* e, uint32_t mirror_limit, uint32_t x0,
                    uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride);

// The additional conditions of the variance calls (name: mm_trace_tile_var / mm_trace_pixels_var /
// mm_trace_pixel_lists): at least two samples, no accumulation, and a variance buffer of n floats apart from
// the output's out_bytes.
ArgCheck check_var(const char* name, const mm_ext* e, const void* out_dev, uint64_t out_bytes, const float* var_dev,
                   uint64_t n);

// mm_trace_tile, _frames, _cameras and _var.  The shared checks say "mm_trace_tile:" whichever entry point was
// used; "no frames" carries multi_fn, the multi-frame entry point's name (mm_trace_tile_frames, or
// mm_trace_tile_cameras with cameras); var: mm_trace_tile_var, whose conditions carry its own name.
ArgCheck check_trace_tile(const char* multi_fn, bool var, const mm_uniform* u, const mm_ext* e, uint32_t n_frames,
                          uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, const void* out_dev,
                          const float* var_dev);

// mm_trace_pixels and _var (lists false: one list, offsets = {0, n_pixels}; the shared checks say
// "mm_trace_pixels:", the variance conditions "mm_trace_pixels_var:") and mm_trace_pixel_lists (lists true: its
// offsets are checked first, mm_plan.h lists_total; every message carries its name).  n_entries: the entries of
// all lists.  MM_OK with n_entries == 0 is the call that has nothing to do: no other check is then made.
ArgCheck check_trace_lists(bool lists, bool var, const mm_uniform* u, const mm_ext* e, const uint64_t* offsets,
                           uint32_t n_lists, const uint32_t* pixels_dev, const void* out_dev, const float* var_dev,
                           uint64_t& n_entries);

// mm_trace_rays, in the order include/mm_api.h states: MM_OK with n_rays == 0 (nothing else checked); a null
// ext, rays_dev or out_dev; a misaligned rays_dev (16 bytes) or out_dev (16, or 4 with MM_EXT_RGBA8); unknown
// ray_flags; spp, then the limits, out of range; MM_EXT_RGBA8 with MM_EXT_ACCUMULATE; with var_dev, the variance
// conditions (check_var, under the call's own name; a misaligned var_dev is found there).  The queue and staging
// bounds are the plan's (mm_plan.h plan_rays), which the call consults next.
ArgCheck check_trace_rays(const mm_ext* e, uint32_t ray_flags, const float* rays_dev, uint64_t n_rays,
                          const void* out_dev, const float* var_dev);

// mm_trace_aov.  has_cams: the call came with cameras.
ArgCheck check_trace_aov(const mm_uniform* u, bool has_cams, uint32_t n_frames, uint32_t mirror_limit, uint32_t x0,
                         uint32_t y0, uint32_t w, uint32_t h, uint32_t y_stride, const mm_aov* out);

// mm_query_rays.  max_rays: what one launch holds (mm_aov.h aov_max_items).  MM_OK with n_rays == 0: nothing to
// do, and nothing else checked.
ArgCheck check_query_rays(const float* rays_dev, uint64_t n_rays, const void* hits_dev, uint64_t max_rays);

}  // namespace mm
