// temporal_var_kernels.hip — mm_accumulate_frames_var and mm_blend_pixels_var (include/mm_api.h states the
// arithmetic; tests/temporal_var_ref.c restates it in plain C and the GPU result equals it bit for bit).
//
//   k_temporal_frame_var  k_temporal_frame (temporal_kernels.hip) with the variance of the pixel mean
//                         carried beside the colour and a per-pixel frame weight: the same 64 x 4 blocks,
//                         one thread per pixel, the same reprojection (mm_temporal.h) and the same
//                         branch-free taps -- clamped addresses, unconditional in-bounds loads, and
//                         `take ? new : old` selects, so a refuted tap reaches no accumulator, the
//                         variance's included.  Each tap loads one more float (the history variance), the
//                         pixel one or two more (its vmean, its weight) and stores one more: 132 B per
//                         pixel beside the parent's 120, 136 with weights.  kWeights = false is an
//                         instantiation of its own: it loads no weights and m is the constant 1.0f.
//   k_blend_pixels_var    k_blend_pixels with the variance image updated beside the colour.
//
// One launch per frame in stream order, as the parent call: frame f reads the colour and the variance frame
// f - 1's launch wrote, and no thread reads a pixel of its own launch's outputs.
#include <hip/hip_runtime.h>

#include "mm_launch.h"
#include "mm_temporal.h"
#include "mm_trace.h"

namespace mm {

namespace {

// The history of pixel (i, j), whose colour is C, id idp, weight m and variance Vc: false for NOHIST (o and
// vo are then untouched).
template <bool kWeights>
__device__ __forceinline__ bool tp_history_var(const TpFrameVar& b, uint32_t i, uint32_t j, uint32_t p,
                                               const float4& C, uint32_t idp, float m, float Vc, float4& o,
                                               float& vo) {
    const TpFrame& a = b.f;
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
        const float Vq = b.h_var[q];
        const bool take = tp_key(a, in, idq, idp, mhq, mhp, ndp, ndq, dp);
        const float g = (dx ? fa : 1.0f - fa) * (dy ? fb : 1.0f - fb);
        const float nx = Sx + g * Hq.x, ny = Sy + g * Hq.y, nz = Sz + g * Hq.z, nn = SN + g * Hq.w, nw = W + g;
        const float nv = SV + (g * g) * Vq;
        Sx = take ? nx : Sx;
        Sy = take ? ny : Sy;
        Sz = take ? nz : Sz;
        SN = take ? nn : SN;
        SV = take ? nv : SV;
        W = take ? nw : W;
    }
    if (!(W >= a.w_min)) return false;
    const float hx = Sx / W, hy = Sy / W, hz = Sz / W;
    const float VH = SV / (W * W);
    const float N = fminf(SN / W + m, fmaxf(a.n_max, m));
    o = make_float4(hx + ((C.x - hx) * m) / N, hy + ((C.y - hy) * m) / N, hz + ((C.z - hz) * m) / N, N);
    const float bw = m / N, cw = 1.0f - bw;
    vo = (cw * cw) * VH + (bw * bw) * Vc;
    return true;
}

template <bool kWeights>
__global__ __launch_bounds__(256) void k_temporal_frame_var(const TpFrameVar b) {
    const TpFrame& a = b.f;
    const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const uint32_t i = tx * 64 + threadIdx.x;  // (tiles_x * 64 < w + 64)
    const uint32_t j = ty * 4 + threadIdx.y;
    if (i >= a.w || j >= a.h) return;
    const uint32_t p = j * a.w + i;
    const float4 C = a.color[p];
    const float m = kWeights ? b.weight[p] : 1.0f;
    const float Vc = b.vmean[p];
    float4 o = make_float4(C.x, C.y, C.z, m);
    float vo = Vc;
    if (a.h_color) {
        const uint32_t idp = a.id[p];
        if (idp != MM_AOV_ID_MISS && idp != MM_AOV_ID_FAILED)
            (void)tp_history_var<kWeights>(b, i, j, p, C, idp, m, Vc, o, vo);
    }
    a.out[p] = o;
    b.vout[p] = vo;
}

// mm_blend_pixels_var (include/mm_api.h): k_blend_pixels, and the pixel's variance beside it; one lane per
// entry.  An entry outside the window touches nothing (p is computed only inside it: p < w * h < 2^31).
__global__ __launch_bounds__(256) void k_blend_pixels_var(const TpBlendVar v) {
    const TpBlend& b = v.b;
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
    const float bw = b.m / Nn, cw = 1.0f - bw;
    v.var[p] = (cw * cw) * v.var[p] + (bw * bw) * v.extra_vmean[e];
}

}  // namespace

hipError_t launch_blend_pixels_var(const TpBlendVar& blend, hipStream_t s) {
    const uint64_t blocks = (blend.b.n + 255) / 256;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_blend_pixels_var, dim3((unsigned)blocks), dim3(256), 0, s, blend);
    return hipGetLastError();
}

hipError_t launch_temporal_frame_var(const TpFrameVar& frame, hipStream_t s) {
    TpFrameVar b = frame;
    b.f.tiles_x = (b.f.w + 63) / 64;
    const uint64_t tiles = (uint64_t)b.f.tiles_x * ((b.f.h + 3) / 4);
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (b.weight)
        hipLaunchKernelGGL(k_temporal_frame_var<true>, dim3((unsigned)tiles), dim3(64, 4), 0, s, b);
    else
        hipLaunchKernelGGL(k_temporal_frame_var<false>, dim3((unsigned)tiles), dim3(64, 4), 0, s, b);
    return hipGetLastError();
}

}  // namespace mm
