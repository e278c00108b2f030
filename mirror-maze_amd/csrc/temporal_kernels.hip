// temporal_kernels.hip — the temporal accumulation of mm_accumulate_frames and
// mm_blend_pixels, and of their variance forms mm_accumulate_frames_var and
// mm_blend_pixels_var (include/mm_api.h states the arithmetic; tests/temporal_ref.c
// and tests/temporal_var_ref.c restate it in plain C and the GPU result equals
// them bit for bit).  One source for both: the kernels and tp_history are
// templates over kVar, and what the variance calls add stands under
// `if constexpr (kVar)`.
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
// The rotation, the projection, a tap's address and the key test are mm_temporal.h's.
//
//   kVar              (mm_accumulate_frames_var) the variance of the pixel mean carried beside the colour,
//                     and a per-pixel frame weight: the same blocks, the same reprojection and the same
//                     branch-free taps -- clamped addresses, unconditional in-bounds loads, and
//                     `take ? new : old` selects, so a refuted tap reaches no accumulator, the variance's
//                     included.  Each tap loads one more float (the history variance), the pixel one or
//                     two more (its vmean, its weight) and stores one more: 132 B per pixel beside the
//                     plain kernel's 120, 136 with weights.  kWeights = false is an instantiation of its
//                     own: it loads no weights and m is the constant 1.0f.  The plain instance keeps its
//                     own arithmetic (+ 1.0f, n_max, no product with m): it is not the variance form at m = 1.
//   k_blend_pixels    kVar: the variance image updated beside the colour.
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

#include <type_traits>

#include "mm_launch.h"
#include "mm_temporal.h"
#include "mm_trace.h"

namespace mm {

namespace {

// A kernel's argument: the plain struct, or the variance call's, which holds one first (mm_launch.h).
template <bool kVar>
using TpFrameArgs = std::conditional_t<kVar, TpFrameVar, TpFrame>;
template <bool kVar>
using TpBlendArgs = std::conditional_t<kVar, TpBlendVar, TpBlend>;
__device__ __forceinline__ const TpFrame& tp_frame(const TpFrame& a) { return a; }
__device__ __forceinline__ const TpFrame& tp_frame(const TpFrameVar& b) { return b.f; }
__device__ __forceinline__ const TpBlend& tp_blend(const TpBlend& b) { return b; }
__device__ __forceinline__ const TpBlend& tp_blend(const TpBlendVar& v) { return v.b; }

// The history of pixel (i, j), whose colour is C and id idp -- and, kVar, weight m and variance Vc: false for
// NOHIST (o and vo are then untouched).
template <bool kVar, bool kWeights>
__device__ __forceinline__ bool tp_history(const TpFrameArgs<kVar>& b, uint32_t i, uint32_t j, uint32_t p,
                                           const float4& C, uint32_t idp, float m, float Vc, float4& o, float& vo) {
    const TpFrame& a = tp_frame(b);
    const float4 ndp = a.nd[p];
    const float mhp = a.al[p].w;
    float uu, vv, dp;
    if (!tp_project(a, i, j, ndp.w, uu, vv, dp)) return false;
    // (uu in [-1, w), vv in [-1, h), w and h at most 2^24: the conversions are exact and i0 + 1 <= w, j0 + 1 <= h)
    const float fu = floorf(uu), fv = floorf(vv);
    const float fa = uu - fu, fb = vv - fv;
    const int i0 = (int)fu, j0 = (int)fv;
    float Sx = 0.0f, Sy = 0.0f, Sz = 0.0f, SN = 0.0f, SV = 0.0f, W = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int dx = t & 1, dy = t >> 1;
        bool in;
        const uint32_t q = tp_tap(a, i0 + dx, j0 + dy, in);
        const float4 Hq = a.h_color[q];
        const float4 ndq = a.h_nd[q];
        const float mhq = a.h_al[q].w;
        const uint32_t idq = a.h_id[q];
        float Vq = 0.0f;
        if constexpr (kVar) Vq = b.h_var[q];
        const bool take = tp_key(a, in, idq, idp, mhq, mhp, ndp, ndq, dp);
        const float g = (dx ? fa : 1.0f - fa) * (dy ? fb : 1.0f - fb);
        const float nx = Sx + g * Hq.x, ny = Sy + g * Hq.y, nz = Sz + g * Hq.z, nn = SN + g * Hq.w, nw = W + g;
        float nv = 0.0f;
        if constexpr (kVar) nv = SV + (g * g) * Vq;
        Sx = take ? nx : Sx;
        Sy = take ? ny : Sy;
        Sz = take ? nz : Sz;
        SN = take ? nn : SN;
        if constexpr (kVar) SV = take ? nv : SV;
        W = take ? nw : W;
    }
    if (!(W >= a.w_min)) return false;
    const float hx = Sx / W, hy = Sy / W, hz = Sz / W;
    if constexpr (kVar) {
        const float VH = SV / (W * W);
        const float N = fminf(SN / W + m, fmaxf(a.n_max, m));
        o = make_float4(hx + ((C.x - hx) * m) / N, hy + ((C.y - hy) * m) / N, hz + ((C.z - hz) * m) / N, N);
        const float bw = m / N, cw = 1.0f - bw;
        vo = (cw * cw) * VH + (bw * bw) * Vc;
    } else {
        const float N = fminf(SN / W + 1.0f, a.n_max);
        o = make_float4(hx + (C.x - hx) / N, hy + (C.y - hy) / N, hz + (C.z - hz) / N, N);
    }
    return true;
}

template <bool kVar, bool kWeights>
__global__ __launch_bounds__(256) void k_temporal_frame(const TpFrameArgs<kVar> b) {
    const TpFrame& a = tp_frame(b);
    const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const uint32_t i = tx * 64 + threadIdx.x;  // (tiles_x * 64 < w + 64)
    const uint32_t j = ty * 4 + threadIdx.y;
    if (i >= a.w || j >= a.h) return;
    const uint32_t p = j * a.w + i;
    const float4 C = a.color[p];
    float m = 1.0f, Vc = 0.0f;
    if constexpr (kVar) {
        if constexpr (kWeights) m = b.weight[p];
        Vc = b.vmean[p];
    }
    float4 o = make_float4(C.x, C.y, C.z, m);
    float vo = Vc;
    if (a.h_color) {
        const uint32_t idp = a.id[p];
        if (idp != MM_AOV_ID_MISS && idp != MM_AOV_ID_FAILED)
            (void)tp_history<kVar, kWeights>(b, i, j, p, C, idp, m, Vc, o, vo);
    }
    a.out[p] = o;
    if constexpr (kVar) b.vout[p] = vo;
}

// mm_blend_pixels / mm_blend_pixels_var (include/mm_api.h): entry e's extra samples into its pixel of the
// accumulated window, in place -- kVar: and the pixel's variance beside it; one lane per entry.  An entry outside
// the window touches nothing (p is computed only inside it: p < w * h < 2^31).
template <bool kVar>
__global__ __launch_bounds__(256) void k_blend_pixels(const TpBlendArgs<kVar> v) {
    const TpBlend& b = tp_blend(v);
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
    if constexpr (kVar) {
        const float bw = b.m / Nn, cw = 1.0f - bw;
        v.var[p] = (cw * cw) * v.var[p] + (bw * bw) * v.extra_vmean[e];
    }
}

template <bool kVar>
hipError_t launch_blend(const TpBlendArgs<kVar>& v, uint64_t n, hipStream_t s) {
    const uint64_t blocks = (n + 255) / 256;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_blend_pixels<kVar>, dim3((unsigned)blocks), dim3(256), 0, s, v);
    return hipGetLastError();
}

// (a: b's TpFrame)
template <bool kVar>
hipError_t launch_frame(TpFrameArgs<kVar>& b, TpFrame& a, hipStream_t s) {
    a.tiles_x = (a.w + 63) / 64;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.h + 3) / 4);
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles), block(64, 4);
    if constexpr (kVar) {
        if (b.weight) hipLaunchKernelGGL((k_temporal_frame<true, true>), grid, block, 0, s, b);
        else hipLaunchKernelGGL((k_temporal_frame<true, false>), grid, block, 0, s, b);
    } else {
        hipLaunchKernelGGL((k_temporal_frame<false, false>), grid, block, 0, s, b);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_blend_pixels(const TpBlend& blend, hipStream_t s) { return launch_blend<false>(blend, blend.n, s); }
hipError_t launch_blend_pixels_var(const TpBlendVar& blend, hipStream_t s) {
    return launch_blend<true>(blend, blend.b.n, s);
}

hipError_t launch_temporal_frame(const TpFrame& frame, hipStream_t s) {
    TpFrame a = frame;
    return launch_frame<false>(a, a, s);
}
hipError_t launch_temporal_frame_var(const TpFrameVar& frame, hipStream_t s) {
    TpFrameVar b = frame;
    return launch_frame<true>(b, b.f, s);
}

}  // namespace mm
