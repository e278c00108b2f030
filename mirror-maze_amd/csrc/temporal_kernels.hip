// temporal_kernels.hip — the temporal accumulation of mm_accumulate_frames
// (include/mm_api.h states the arithmetic; tests/temporal_ref.c restates it in
// plain C and the GPU result equals it bit for bit).
//
//   k_temporal_frame  one frame: one thread per output pixel, 64 x 4 blocks as
//                     k_denoise_pass, so a wave is a 64-pixel row segment.  The
//                     pixel's virtual image (camera centre + distance along the
//                     mirror chain * its primary direction) is projected into
//                     the history frame's camera; the four pixels around the
//                     projection are the taps.  Under smooth motion the wave's
//                     taps are row segments of the history frame shifted by
//                     the motion: near-coherent gathers, which measured no
//                     slower than taps that fall exactly on their own pixels
//                     (profiles/temporal/ab.txt).
//
// The rotation, the projection, a tap's address and the key test are mm_temporal.h's, shared with
// k_temporal_frame_var (temporal_var_kernels.hip), which runs the same reprojection.
//
// Frame f reads what frame f - 1's launch wrote, so a call is one launch per
// frame in stream order: the kernel boundary is what makes frame f - 1's
// stores visible, and no thread reads a pixel of its own launch's output.
//
// The taps are branch-free, as the denoiser's: addresses are clamped into the
// frame, every load is unconditional and in bounds, and a tap outside the tile
// or refuted by the key test is computed and not added (a select, not a zero
// weight: the accumulators never see it).  The thirteen divisions and the square
// root of a pixel are the compiler's correctly rounded sequences (the build's
// default): at about 250 VALU operations per pixel beside 120 B of HBM traffic
// the kernel is not VALU-bound the way the denoiser's 25-tap pass was, so the
// guarded Markstein quotients and their second, exact form are not worth their
// code here (DESIGN.md §4 "Temporal accumulation").
#include <hip/hip_runtime.h>

#include "mm_launch.h"
#include "mm_temporal.h"
#include "mm_trace.h"

namespace mm {

namespace {

// The history of pixel (i, j), whose colour is C and id idp: false for NOHIST (o is then untouched).
__device__ __forceinline__ bool tp_history(const TpFrame& a, uint32_t i, uint32_t j, uint32_t p, const float4& C,
                                           uint32_t idp, float4& o) {
    const float4 ndp = a.nd[p];
    const float mhp = a.al[p].w;
    float uu, vv, dp;
    if (!tp_project(a, i, j, ndp.w, uu, vv, dp)) return false;
    // (uu in [-1, w), vv in [-1, h), w and h at most 2^24: the conversions are exact and i0 + 1 <= w, j0 + 1 <= h)
    const float fu = floorf(uu), fv = floorf(vv);
    const float fa = uu - fu, fb = vv - fv;
    const int i0 = (int)fu, j0 = (int)fv;
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, SN = 0.0f, W = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int dx = t & 1, dy = t >> 1;
        bool in;
        const uint32_t q = tp_tap(a, i0 + dx, j0 + dy, in);
        const float4 Hq = a.h_color[q];
        const float4 ndq = a.h_nd[q];
        const float mhq = a.h_al[q].w;
        const uint32_t idq = a.h_id[q];
        const bool take = tp_key(a, in, idq, idp, mhq, mhp, ndp, ndq, dp);
        const float g = (dx ? fa : 1.0f - fa) * (dy ? fb : 1.0f - fb);
        const float nx = Sx + g * Hq.x, ny = Sy + g * Hq.y, nz = Sz + g * Hq.z, nn = SN + g * Hq.w, nw = W + g;
        Sx = take ? nx : Sx;
        Sy = take ? ny : Sy;
        Sz = take ? nz : Sz;
        SN = take ? nn : SN;
        W = take ? nw : W;
    }
    if (!(W >= a.w_min)) return false;
    const float hx = Sx / W, hy = Sy / W, hz = Sz / W;
    const float N = fminf(SN / W + 1.0f, a.n_max);
    o = make_float4(hx + (C.x - hx) / N, hy + (C.y - hy) / N, hz + (C.z - hz) / N, N);
    return true;
}

__global__ __launch_bounds__(256) void k_temporal_frame(const TpFrame a) {
    const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const uint32_t i = tx * 64 + threadIdx.x;  // (tiles_x * 64 < w + 64)
    const uint32_t j = ty * 4 + threadIdx.y;
    if (i >= a.w || j >= a.h) return;
    const uint32_t p = j * a.w + i;
    const float4 C = a.color[p];
    float4 o = make_float4(C.x, C.y, C.z, 1.0f);
    if (a.h_color) {
        const uint32_t idp = a.id[p];
        if (idp != MM_AOV_ID_MISS && idp != MM_AOV_ID_FAILED) (void)tp_history(a, i, j, p, C, idp, o);
    }
    a.out[p] = o;
}

// mm_blend_pixels (include/mm_api.h): entry e's extra samples into its pixel of the accumulated window, in
// place; one lane per entry.  An entry outside the window touches nothing (p is computed only inside it:
// p < w * h < 2^31).
__global__ __launch_bounds__(256) void k_blend_pixels(const TpBlend b) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b.n) return;
    const uint2 r = b.pixels[e];
    if (r.x < b.x0 || r.x - b.x0 >= b.w || r.y < b.y0 || r.y - b.y0 >= b.h) return;
    const uint32_t p = (r.y - b.y0) * b.w + (r.x - b.x0);
    const float4 A = b.image[p];
    const float4 E = b.extra[e];
    const float Nn = A.w + b.m;
    b.image[p] = make_float4(A.x + ((E.x - A.x) * b.m) / Nn, A.y + ((E.y - A.y) * b.m) / Nn,
                             A.z + ((E.z - A.z) * b.m) / Nn, Nn);
}

}  // namespace

hipError_t launch_blend_pixels(const TpBlend& blend, hipStream_t s) {
    const uint64_t blocks = (blend.n + 255) / 256;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_blend_pixels, dim3((unsigned)blocks), dim3(256), 0, s, blend);
    return hipGetLastError();
}

hipError_t launch_temporal_frame(const TpFrame& frame, hipStream_t s) {
    TpFrame a = frame;
    a.tiles_x = (a.w + 63) / 64;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.h + 3) / 4);
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_temporal_frame, dim3((unsigned)tiles), dim3(64, 4), 0, s, a);
    return hipGetLastError();
}

}  // namespace mm
